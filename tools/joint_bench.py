"""The joint count spectrum and the joint count-window filter against existing code reading the same bytes, in one process.

    python tools/joint_bench.py [--reads 20000000 --k 63 --m 21 --b 14] [--part-bits 0] [--reps 5] [--host-route]

Two indexes A and B from the two halves of bench.py's read set, as tools/setops_bench.py builds them.  Every measured call is
synchronous, so the host clock around it is the kernels plus launches, a copy (528 KB for the matrix) and a stream
synchronisation.  Medians of --reps alternating rounds, with every value.  filter_joint and intersect change A: they run on a
rebuilt A (clear + insert_packed, not timed).
  compare_ms + count_spectrum_b_ms   the yardstick of joint_spectrum: existing, unchanged code that reads the same keys and counts
  joint_spectrum_ms                  brisk_hip_joint_spectrum(A, B)
  intersect_left_ms                  the yardstick of filter_joint
  filter_joint_ms                    brisk_hip_filter_joint(A, B, {0,255, 0,255, 0}): the same survivors
  filter_window_ms                   brisk_hip_filter_joint(A, B, {2,255, 0,1, absent}): solid here, absent or a singleton there
  --host-route                       once: enumerate both to the host and joint_spectrum_from_entries (wall time)
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
from tools.setops_bench import stat, timed  # noqa: E402


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
    keys = ("compare", "count_spectrum_b", "joint_spectrum", "intersect_left", "filter_joint", "filter_window")
    ms = {key: [] for key in keys}
    absent = brisk_amd.JOINT_ABSENT
    for rep in range(a.reps + 1):  # the first round warms up
        row = {}
        row["compare"], cmp_ = timed(lambda: A.compare(B))
        row["count_spectrum_b"], spec_b = timed(B.count_spectrum)
        row["joint_spectrum"], J = timed(lambda: A.joint_spectrum(B))
        row["intersect_left"], n_int = timed(lambda: A.intersect(B, count="left"))
        cs_int = A.checksum()
        build(A, 0)
        row["filter_joint"], n_flt = timed(lambda: A.filter_joint(B))
        cs_flt = A.checksum()
        build(A, 0)
        row["filter_window"], n_win = timed(lambda: A.filter_joint(B, 2, 255, 0, 1, keep_absent=True))
        cs_win = A.checksum()
        build(A, 0)
        # the results agree with each other; A and B are what they were
        assert A.checksum() == cs_a and B.checksum() == cs_b
        assert np.array_equal(J[:absent].sum(axis=1), A.count_spectrum()) and np.array_equal(J[:, :absent].sum(axis=0), spec_b)
        assert int(J[:absent, :absent].sum()) == cmp_["both"] and int(J[:absent, absent].sum()) == cmp_["only_self"] and int(J[absent, :absent].sum()) == cmp_["only_other"]
        assert n_flt == n_int and cs_flt == cs_int
        assert cs_win[0] == cs_a[0] - n_win == int(J[2:absent, absent].sum() + J[2:absent, :2].sum())
        if rep:
            for key in keys:
                ms[key].append(row[key])
    res["compare"] = cmp_
    res["joint_nonzero_bins"] = int(np.count_nonzero(J))
    res["joint_top_bins"] = [[int(i // 257), int(i % 257), int(J.flat[i])] for i in np.argsort(J, axis=None)[::-1][:6]]
    res["figures"] = brisk_amd.joint_figures(J, a.k)
    res["filter_window_removed"] = n_win
    for key in keys:
        res[key + "_ms"] = stat(ms[key])
    yard = res["compare_ms"]["median"] + res["count_spectrum_b_ms"]["median"]
    res["compare_plus_spectrum_b_ms"] = round(yard, 3)
    res["joint_spectrum_over_yardstick"] = round(res["joint_spectrum_ms"]["median"] / yard, 3)
    res["filter_joint_over_intersect"] = round(res["filter_joint_ms"]["median"] / res["intersect_left_ms"]["median"], 3)
    if a.host_route:
        t0 = time.perf_counter()
        ea, eb = A.enumerate(chunk=1 << 26), B.enumerate(chunk=1 << 26)
        t1 = time.perf_counter()
        host = brisk_amd.joint_spectrum_from_entries(ea, eb)
        t2 = time.perf_counter()
        assert np.array_equal(host, J)
        res["host_route"] = {"enumerate_both_s": round(t1 - t0, 2), "numpy_join_s": round(t2 - t1, 2), "bytes_over_pcie": (len(ea[0]) + len(eb[0])) * 18}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
