"""Paired-end extraction on the bench's workload: N synthetic 150 bp reads at 15x coverage (k63 m21 b14 by default: bench.py's),
resident on the device as a packed stream, inserted, and taken as N / 2 interleaved pairs, then

  1. brisk_hip_trim_pairs_packed (pair mode each, solid_run, solid_min 2) against brisk_hip_trim_packed on the same reads in the
     same process, alternating, host clocks around synchronised calls, the first pair a warm-up, medians: what keeping the mates
     in sync costs on top of trimming them;
  2. brisk_hip_extract_pairs_packed alone against brisk_hip_extract_packed over the same kept set, on given intervals
     ([--start, --start + --len) of two reads in three: one pair in three stays intact, the other two leave a single each).

The byte model of the pair work: k_pair_split reads the intervals (8 B a read) and the read table (8 B a read: the validity check
that lets the call refuse before either stream is written) and writes two masked tables (16 B a read); the second gather reads the
read table and its masked table once more in each of its two table passes.  Checks the two streams of case 2 against the single
stream of extract_packed through the indexes, and times extract_packed over each of the two masked tables on its own, so that the
pairs call's time splits into the two gathers and the split pass.  Prints one JSON line.

    python tools/pairs_bench.py [--reads 50000000] [--reps 5] [--k 63 --m 21 --b 14] [--solid 2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import brisk_amd  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=63)
    ap.add_argument("--m", type=int, default=21)
    ap.add_argument("--b", type=int, default=14)
    ap.add_argument("--part-bits", type=int, default=0)
    ap.add_argument("--coverage", type=float, default=15.0)
    ap.add_argument("--solid", type=int, default=2)
    ap.add_argument("--start", type=int, default=7)
    ap.add_argument("--len", type=int, default=120)
    a = ap.parse_args()
    n, L = a.reads // 2 * 2, 150
    assert a.start + a.len <= L
    G = max(int(n * L / a.coverage), L + 1)
    dev = torch.device("cuda", 0)
    n_words = (n * L + 15) // 16
    d_packed = torch.zeros(n_words + 4, dtype=torch.int32, device=dev)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)

    class Out:  # one output stream
        def __init__(self):
            self.packed = torch.zeros(n_words + 4, dtype=torch.int32, device=dev)
            self.starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            self.index = torch.zeros(n, dtype=torch.int64, device=dev)

        def args(self):
            return self.packed.data_ptr(), n_words + 4, self.starts.data_ptr(), self.index.data_ptr()

    one, pairs, singles = Out(), Out(), Out()
    torch.cuda.synchronize()  # torch fills on its own stream, the library works on another
    ix = brisk_amd.BriskHip(a.k, a.m, a.b, part_bits=a.part_bits)
    ix.synth_reads(G, 0, n, L, d_packed.data_ptr(), d_starts.data_ptr())
    ix.sync()
    ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
    ix.sync()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    med = lambda v: sorted(v)[len(v) // 2]
    rnd = lambda v: [round(x, 3) for x in v]
    stat = lambda v: {"median": round(med(v), 3), "all": rnd(v)}
    rule = brisk_amd.select_rule("solid_run")
    got = {}

    # ---- 1: trim_pairs_packed against trim_packed
    def trim():
        got["trim"] = ix.trim_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, *one.args(), a.solid, rule)

    def trim_pairs():
        got["trim_pairs"] = ix.trim_pairs_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, pairs.args(), singles.args(), a.solid, rule, "each")

    trim_ms, pairs_ms = [], []
    for rep in range(a.reps + 1):  # the first pair warms up (allocations)
        t, p = timed(trim), timed(trim_pairs)
        if rep:
            trim_ms.append(t)
            pairs_ms.append(p)
    c = got["trim_pairs"]
    same_kept = got["trim"] == (2 * c["n_pairs_kept"] + c["n_single_first"] + c["n_single_second"], c["n_nts_pairs"] + c["n_nts_singles"])

    # ---- 2: extract_pairs_packed alone against extract_packed over the same kept set
    d_iv = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    keep = (torch.arange(n, device=dev) % 3) != 0
    d_iv[:, 0] = torch.where(keep, a.start, 0)
    d_iv[:, 1] = torch.where(keep, a.len, 0)
    del keep
    torch.cuda.synchronize()

    def extract():
        got["extract"] = ix.extract_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_iv.data_ptr(), *one.args())

    def extract_pairs():
        got["extract_pairs"] = ix.extract_pairs_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_iv.data_ptr(), pairs.args(), singles.args())

    ex_ms, exp_ms = [], []
    for rep in range(a.reps + 1):
        t, p = timed(extract), timed(extract_pairs)
        if rep:
            ex_ms.append(t)
            exp_ms.append(p)
    c2 = got["extract_pairs"]
    # where the pairs call's time goes: extract_packed over each of the two masked tables (made here with torch) is what the call runs
    # after k_pair_split; the rest is the split pass, its counters' way to the host and the capacity check
    both = (d_iv[0::2, 1] != 0) & (d_iv[1::2, 1] != 0)
    d_tab = {}
    for name, mask in (("pairs_table", both), ("singles_table", ~both)):
        d_tab[name] = d_iv * mask.repeat_interleave(2).unsqueeze(1).to(torch.int32)
    del both
    torch.cuda.synchronize()
    parts = {}
    for name, out in (("pairs_table", pairs), ("singles_table", singles)):
        ms = [timed(lambda: ix.extract_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_tab[name].data_ptr(), *out.args())) for _ in range(a.reps + 1)][1:]
        parts["extract_packed_over_" + name + "_ms"] = stat(ms)
    parts["split_pass_and_host_round_trip_ms"] = round(med(exp_ms) - sum(v["median"] for v in parts.values()), 3)
    del d_tab
    n_p, n_s = 2 * c2["n_pairs_kept"], c2["n_single_first"] + c2["n_single_second"]
    # the two streams hold, between them, the reads of the one: the indexes merged are the one stream's index
    merged = torch.sort(torch.cat([pairs.index[:n_p], singles.index[:n_s]])).values
    checks = {"counts_add_up": got["extract"] == (n_p + n_s, c2["n_nts_pairs"] + c2["n_nts_singles"]),
              "indexes_partition_the_kept_reads": bool(torch.equal(merged, one.index[:n_p + n_s])),
              "pairs_are_interleaved": bool((pairs.index[0:n_p:2] + 1 == pairs.index[1:n_p:2]).all())}
    del merged
    # the pair work by the byte model: one pass of k_pair_split, and the two table passes of the second gather
    split_b = n * (8 + 8) + n * 16
    second_tables_b = 2 * n * 16
    res = {"tool": "pairs_bench", "config": {"reads": n, "pairs": n // 2, "read_len": L, "k": a.k, "m": a.m, "b": a.b, "coverage": a.coverage, "solid_min": a.solid, "reps": a.reps},
           "entries": ix.stats()["nb_kmers"],
           "trim_packed_ms": stat(trim_ms), "trim_pairs_packed_ms": stat(pairs_ms),
           "trim_pairs_over_trim": round(med(pairs_ms) / med(trim_ms), 4), "trim_pairs_minus_trim_ms": round(med(pairs_ms) - med(trim_ms), 3),
           "trim_kept": list(got["trim"]), "trim_pairs_counts": c, "trim_pairs_keeps_what_trim_keeps": same_kept,
           "extract_alone": {"intervals": "[%d, %d) of two reads in three" % (a.start, a.start + a.len), "extract_packed_ms": stat(ex_ms), "extract_pairs_packed_ms": stat(exp_ms),
                             "pairs_over_single": round(med(exp_ms) / med(ex_ms), 4), "pairs_minus_single_ms": round(med(exp_ms) - med(ex_ms), 3), "counts": c2, "parts": parts, "checks": checks},
           "byte_model": {"pair_split_bytes": split_b, "second_gather_table_bytes": second_tables_b,
                          "added_ms_at_4_TB_per_s": round((split_b + second_tables_b) / 4e9, 3)}}
    print(json.dumps(res))
    ix.close()
    return 0 if same_kept and all(checks.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
