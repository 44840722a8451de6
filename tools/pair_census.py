"""Census of the pair rule of k_insert_first, on the CPU (DESIGN.md section 4 finding 22).
    python tools/pair_census.py [READS]        (default 60000; k63 m21 b14)
Runs tests/insert_pair_rules.py over the oracle's records of two read sets at the flagship job's density -- the bench's synthetic
reads (genome of 10 positions per read) and the error-bearing reads of tests/density_reads.py -- with the partition width scaled so
that a partition holds about 12.5 records, as the 50 M read job's 2^24 partitions do.  The touched list is walked in ascending
order, batches of 64.  Prints what profiles/r25_pair_census.txt keeps."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import oracle
import fold_group_rules as G
import insert_pair_rules as PR
from density_reads import dense_reads, _offsets

reads = int(sys.argv[1]) if len(sys.argv) > 1 else 60000
oracle.build(ref=False)
O = oracle.Oracle()


def census(name, data):
    # the width at which the touched partitions hold closest to 12.5 records (tools/fold_census.py)
    base, best = G.partitions_of(O, data, 4), (1e9, None, None)
    for shift in range(4, 24):
        grouped = {}
        for p, recs in base.items():
            grouped.setdefault(p >> (shift - 4), []).extend(recs)
        mean = sum(len(r) for r in grouped.values()) / len(grouped)
        if abs(mean - 12.5) < best[0]:
            best = (abs(mean - 12.5), shift, grouped)
    _, shift, parts = best
    order, n = sorted(parts), len(parts)
    pct = lambda x: f"{100.0 * x / n:.1f} %"
    print(f"{name}: {len(data[1]) - 1} reads, partition = bucket >> {shift}: {n} partitions touched, {sum(len(r) for r in parts.values()) / n:.2f} records each")
    states = {p: PR.single(r, shift) for p, r in parts.items() if len(r) <= PR.MAX_REC}
    lean = [s for s in states.values() if s[2] <= PR.MAXI]
    print(f"  per partition: instances after the fold {np.mean([s[2] for s in lean]):.1f} (those of at most {PR.MAXI}), clean {pct(sum(s[1] for s in lean))}, "
          f"left over (more than {PR.MAX_REC} records or {PR.MAXI} instances) {pct(n - len(lean))}")
    for need_clean in (True, False):
        out = PR.walk(order, parts, rid_bits=shift, need_clean=need_clean)
        t = PR.tally(out)
        one, two, taken = PR.passes(out, parts, shift)
        print(f"  {'the rule' if need_clean else 'without the clean condition (a table path for pairs)'}: in a pair {pct(t['pair'])}, alone {pct(sum(t['alone'].values()))}, left over {pct(t['left'])}")
        print("    alone by reason: " + ", ".join(f"{r} {pct(c)}" for r, c in t["alone"].items()))
        print(f"    instance passes per partition taken: single scheme {one / taken:.3f}, pair scheme {two / taken:.3f}; wave trips per partition taken {1 - t['pair'] / 2 / taken:.3f}")
        if need_clean:
            both = [(p, o[1]) for p, o in out.items() if o[0] == "pair" and p < o[1]]
            print(f"    a pair: {np.mean([len(parts[a]) + len(parts[b]) for a, b in both]):.1f} records, {np.mean([states[a][2] + states[b][2] for a, b in both]):.1f} instances on average")
    # the joint fold against the per-partition rule, every neighbouring couple that may share a wave
    differ = tried = 0
    for a, b in zip(order, order[1:]):
        if len(parts[a]) + len(parts[b]) <= PR.MAX_REC:
            j = PR.joint(parts[a], parts[b], shift)
            if j is not None:
                tried += 1
                differ += (j[0], j[1], j[2]) != states[a] or (j[3], j[4], j[5]) != states[b]
    print(f"  joint folds that stand: {tried} of {n - 1} neighbouring couples; those where a record's (folded, lead, off) or a partition's clean differs from the per-partition rule: {differ}")


syn = O.synth_reads(reads * 10, 0, reads)
census("synthetic (bench)", (np.ascontiguousarray(syn.reshape(-1)), _offsets(np.full(reads, syn.shape[1], np.int64))))
census("error-bearing (density_reads, e = 0.01)", dense_reads(reads, 63, reads * 10, 1, e=0.01))
