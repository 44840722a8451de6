"""Census of the fold rounds of k_insert_first under its two rules, on the CPU (DESIGN.md section 4 finding 21).
    python tools/fold_census.py [READS]        (default 60000; k63 m21 b14)
Runs tests/fold_group_rules.py over the oracle's records of two read sets at the flagship job's density -- the bench's synthetic
reads (genome of 10 positions per read) and the error-bearing reads of tests/density_reads.py -- with the partition width scaled
so that a partition holds about 12.5 records, as the 50 M read job's 2^24 partitions do.  Prints what profiles/r24_fold_groups_census.txt keeps."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import oracle
import fold_group_rules as G
from density_reads import dense_reads, _offsets

reads = int(sys.argv[1]) if len(sys.argv) > 1 else 60000
oracle.build(ref=False)
O = oracle.Oracle()


def census(name, data):
    # the width at which the touched partitions hold closest to 12.5 records
    base, best = G.partitions_of(O, data, 4), (1e9, None, None)
    for shift in range(4, 24):
        grouped = {}
        for p, recs in base.items():
            grouped.setdefault(p >> (shift - 4), []).extend(recs)
        mean = sum(len(r) for r in grouped.values()) / len(grouped)
        if abs(mean - 12.5) < best[0]:
            best = (abs(mean - 12.5), shift, grouped)
    _, shift, parts = best
    lean = {p: r for p, r in parts.items() if len(r) <= 64}
    seq_r, grp_r, heads, per_group, fell, unsure, over, clean, differ = [], [], [], [], 0, 0, 0, 0, 0
    for p, recs in lean.items():
        fr = G.frames(recs, rid_bits=shift)
        s, g = G.sequential(fr), G.grouped(fr)
        differ += (s[0], s[1]) != (g[0], g[1])
        seq_r.append(s[2])
        grp_r.append(g[2])
        heads.append(s[3])
        fell += g[4]
        unsure += any(f["unsure"] for f in fr)
        clean += s[1]
        survivors = {}
        for f, (folded, _, _) in zip(fr, s[0]):
            if not folded:
                survivors[f["ck"]] = survivors.get(f["ck"], 0) + 1
        per_group += list(survivors.values())
        over += len([1 for r in s[0] if not r[0]]) > G.FOLD_TRIPS
    n = len(lean)
    print(f"{name}: {len(data[1]) - 1} reads, partition = bucket >> {shift}: {len(parts)} partitions touched, {sum(len(r) for r in parts.values()) / len(parts):.2f} records each, "
          f"{n} of at most 64 records")
    print(f"  rounds per partition   sequential {np.mean(seq_r):.3f}   grouped {np.mean(grp_r):.3f}   ratio {np.mean(grp_r) / np.mean(seq_r):.3f}")
    print(f"  grouped rounds histogram (1, 2, 3, 4, 5+): {[int(np.sum(np.array(grp_r) == i)) for i in (1, 2, 3, 4)] + [int(np.sum(np.array(grp_r) >= 5))]}")
    print(f"  heads per partition {np.mean(heads):.3f}; heads per core-key group {np.mean(per_group):.3f} (max {max(per_group)}); groups per partition {len(per_group) / n:.3f}")
    print(f"  partitions with more than 16 heads: {over} ({100.0 * over / n:.3f} %); with an unsure record: {unsure} ({100.0 * unsure / n:.3f} %); "
          f"handed to the sequential rule: {fell} ({100.0 * fell / n:.3f} %)")
    print(f"  clean {100.0 * clean / n:.1f} %; partitions where the two rules differ in (folded, lead, off, clean): {differ}")


syn = O.synth_reads(reads * 10, 0, reads)
census("synthetic (bench)", (np.ascontiguousarray(syn.reshape(-1)), _offsets(np.full(reads, syn.shape[1], np.int64))))
census("error-bearing (density_reads, e = 0.01)", dense_reads(reads, 63, reads * 10, 1, e=0.01))
