"""Set operations of two indexes against existing code reading the same bytes, in one process.

    python tools/setops_bench.py [--reads 20000000 --k 63 --m 21 --b 14] [--part-bits 0] [--reps 5] [--host-route]

Two indexes A and B from the two halves of bench.py's read set (one genome, reads [0, n) and [n, 2n): the true k-mers are
shared at 15x + 15x coverage, the sets differ where coverage leaves gaps).  Every measured call is synchronous, so the host
clock around it is the kernels plus launches, a small copy and a stream synchronisation (~0.1 ms).  Medians of --reps
alternating rounds, with every value.  Operations that change A run on a rebuilt A (clear + insert_packed, not timed).
  checksum_a_ms + checksum_b_ms   brisk_hip_checksum of both: existing code reading the same keys and counts once (the yardstick)
  compare_ms, subtract_ms, intersect_min_ms
  merge_ms                        brisk_hip_merge(A, B)
  insert_b_into_a_ms              insert_packed of B's reads into A: the only device route to the same index there was
  --host-route                    once: enumerate both to the host and join with numpy (wall time)
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import brisk_amd  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stat(v):
    return {"median": round(sorted(v)[len(v) // 2], 3), "min": round(min(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000, help="reads per index")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=63)
    ap.add_argument("--m", type=int, default=21)
    ap.add_argument("--b", type=int, default=14)
    ap.add_argument("--part-bits", type=int, default=0)
    ap.add_argument("--coverage", type=float, default=15.0)
    ap.add_argument("--host-route", action="store_true")
    a = ap.parse_args()
    n, L = a.reads, 150
    G = max(int(2 * n * L / a.coverage), L + 1)
    res = {"workload": "2 x %d synthetic %d bp reads of one genome of %d nt, k=%d m=%d b=%d part_bits=%d" % (n, L, G, a.k, a.m, a.b, a.part_bits)}
    A = brisk_amd.BriskHip(a.k, a.m, a.b, part_bits=a.part_bits, immediate_inserts=True)
    B = brisk_amd.BriskHip(a.k, a.m, a.b, part_bits=a.part_bits, immediate_inserts=True)
    bufs = []
    for first in (0, n):
        d_packed = torch.zeros((n * L + 15) // 16 + 4, dtype=torch.int32, device="cuda")
        d_starts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        A.synth_reads(G, first, n, L, d_packed.data_ptr(), d_starts.data_ptr())
        A.sync()
        bufs.append((d_packed, d_starts))

    def build(ix, which):
        ix.clear()
        ix.insert_packed(bufs[which][0].data_ptr(), bufs[which][1].data_ptr(), n)
        ix.sync()
    build(A, 0)
    build(B, 1)
    cs_a, cs_b = A.checksum(), B.checksum()
    res["entries"] = {"a": cs_a[0], "b": cs_b[0]}
    res["memory_info"] = {"a": A.memory_info(), "b": B.memory_info()}
    keys = ("checksum_a", "checksum_b", "compare", "subtract", "intersect_min", "merge", "insert_b_into_a")
    ms = {key: [] for key in keys}
    for rep in range(a.reps + 1):  # the first round warms up
        row = {}
        row["checksum_a"], _ = timed(A.checksum)
        row["checksum_b"], _ = timed(B.checksum)
        row["compare"], cmp_ = timed(lambda: A.compare(B))
        row["subtract"], n_sub = timed(lambda: A.subtract(B))
        cs_sub = A.checksum()
        build(A, 0)
        row["intersect_min"], n_int = timed(lambda: A.intersect(B, count="min"))
        cs_int = A.checksum()
        build(A, 0)
        row["merge"], n_add = timed(lambda: A.merge(B))
        cs_merge = A.checksum()
        build(A, 0)
        row["insert_b_into_a"], _ = timed(lambda: (A.insert_packed(bufs[1][0].data_ptr(), bufs[1][1].data_ptr(), n), A.sync()))
        cs_both = A.checksum()
        build(A, 0)
        # the results agree with each other and with the route the merge replaces; B is what it was
        assert cs_merge == cs_both and A.checksum() == cs_a and B.checksum() == cs_b
        assert n_sub == cmp_["both"] and n_int == cmp_["only_self"] and n_add == cmp_["only_other"]
        assert cs_sub[0] == cmp_["only_self"] and cs_int[:2] == (cmp_["both"], cmp_["sum_min"])
        if rep:
            for key in keys:
                ms[key].append(row[key])
    res["compare"] = cmp_
    res["merged_entries"] = cs_merge[0]
    for key in keys:
        res[key + "_ms"] = stat(ms[key])
    yard = res["checksum_a_ms"]["median"] + res["checksum_b_ms"]["median"]
    res["checksum_a_plus_b_ms"] = round(yard, 3)
    for key in ("compare", "subtract", "intersect_min"):
        res[key + "_over_checksums"] = round(res[key + "_ms"]["median"] / yard, 3)
    res["merge_over_insert"] = round(res["merge_ms"]["median"] / res["insert_b_into_a_ms"]["median"], 3)
    if a.host_route:
        t0 = time.perf_counter()
        ea, eb = A.enumerate(chunk=1 << 26), B.enumerate(chunk=1 << 26)
        t1 = time.perf_counter()
        dt = [("hi", np.uint64), ("lo", np.uint64), ("idx", np.uint8)]
        ra, rb = np.zeros(len(ea[0]), dt), np.zeros(len(eb[0]), dt)
        for r, e in ((ra, ea), (rb, eb)):
            r["lo"], r["hi"], r["idx"] = e[0], e[1], e[2]
        both = len(np.intersect1d(ra, rb, assume_unique=True))
        t2 = time.perf_counter()
        assert both == cmp_["both"]
        res["host_route"] = {"enumerate_both_s": round(t1 - t0, 2), "numpy_join_s": round(t2 - t1, 2), "bytes_over_pcie": (len(ea[0]) + len(eb[0])) * 18}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
