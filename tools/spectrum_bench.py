"""Count spectrum and prune against k_checksum (existing code: the yardstick) on one index, in one process.

    python tools/spectrum_bench.py [--reads 50000000 --k 63 --m 21 --b 14] [--part-bits 0] [--reps 5] [--host-route] [--error-reads N]

The index is bench.py's: synthetic 150 bp reads at 15x coverage, inserted in one call.  Every measured call is synchronous (it
ends with a small copy to the host and a stream synchronisation), so the host clock around it is the kernel plus the launch and
the copy (~0.1 ms); per-kernel times come from a rocprofv3 --kernel-trace --stats run of this tool.  Medians of --reps.
  checksum_ms           brisk_hip_checksum: 17 B (two-word keys) or 9 B per entry, three 64-bit mixes
  spectrum_ms           brisk_hip_count_spectrum: 1 B per entry
  prune_none_ms         brisk_hip_prune(0, 255): reads the counts, stores nothing
  prune_2_255_ms        brisk_hip_prune(2, 255), once (it changes the index), with the entries removed and the bytes moved
  --host-route          the same answers by the only route there was: enumerate to the host, numpy (once)
  --error-reads N       N error-bearing reads in the manner of case D of tests/density_parity_worker.py (0.1 % substitutions;
                        tests/density_reads.py) in a second index: spectrum, get_packed over the reads before and after prune(2, 255)
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

HBM_GBS = 8000.0  # MI355X peak, for the roofline fraction


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def med(v):
    return sorted(v)[len(v) // 2]


def stat(v):
    return {"median": round(med(v), 3), "all": [round(x, 3) for x in v]}


def measure(ix, reps, key_bytes):
    out = {}
    st = ix.stats()
    n = st["nb_kmers"]
    cks, sps, prs = [], [], []
    for rep in range(reps + 1):  # the first round warms up
        c, cs = timed(ix.checksum)
        s, spec = timed(ix.count_spectrum)
        p, removed = timed(lambda: ix.prune(0, 255))
        assert removed == 0
        if rep:
            cks.append(c); sps.append(s); prs.append(p)
    assert int(spec.sum()) == n == cs[0] and int((spec * np.arange(256, dtype=np.uint64)).sum()) == cs[1]
    out["entries"] = n
    out["spectrum_bins"] = {str(i): int(v) for i, v in enumerate(spec) if v}
    out["checksum_ms"], out["spectrum_ms"], out["prune_none_ms"] = stat(cks), stat(sps), stat(prs)
    gb = lambda per_entry: n * per_entry / 1e9
    out["checksum_GBs"] = round(gb(key_bytes + 1) / (med(cks) / 1e3), 1)
    out["spectrum_GBs"] = round(gb(1) / (med(sps) / 1e3), 1)
    out["spectrum_over_checksum"] = round(med(sps) / med(cks), 3)
    out["prune_none_over_checksum"] = round(med(prs) / med(cks), 3)
    return out, spec


def prune_once(ix, spec, key_bytes):
    n = int(spec.sum())
    gone = int(spec[:2].sum())
    ms, removed = timed(lambda: ix.prune(2, 255))
    assert removed == gone, (removed, gone)
    # bytes: every count read; a survivor behind a removed entry is read (key) and written (key + count); the bitmap rebuild reads
    # one key word per survivor.  Upper bound: all survivors move.
    moved = n + (n - gone) * (2 * key_bytes + 1) + (n - gone) * 8
    return {"ms": round(ms, 3), "removed": removed, "bytes_upper_bound": moved, "GBs_upper_bound": round(moved / 1e9 / (ms / 1e3), 1),
            "hbm_fraction_upper_bound": round(moved / 1e9 / (ms / 1e3) / HBM_GBS, 3), "checksum_after": list(ix.checksum())}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=63)
    ap.add_argument("--m", type=int, default=21)
    ap.add_argument("--b", type=int, default=14)
    ap.add_argument("--part-bits", type=int, default=0)
    ap.add_argument("--coverage", type=float, default=15.0)
    ap.add_argument("--host-route", action="store_true")
    ap.add_argument("--error-reads", type=int, default=0)
    a = ap.parse_args()
    n, L = a.reads, 150
    res = {"workload": "%d synthetic %d bp reads, %gx coverage, k=%d m=%d b=%d part_bits=%d" % (n, L, a.coverage, a.k, a.m, a.b, a.part_bits)}
    if n:
        G = max(int(n * L / a.coverage), L + 1)
        d_packed = torch.zeros((n * L + 15) // 16 + 4, dtype=torch.int32, device="cuda")
        d_starts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ix = brisk_amd.BriskHip(a.k, a.m, a.b, part_bits=a.part_bits)
        key_bytes = 8 if 2 * a.b + ix.layout["ext_bits"] - ix.layout["part_bits"] + 2 * (a.k - a.b) + 6 <= 64 else 16
        ix.synth_reads(G, 0, n, L, d_packed.data_ptr(), d_starts.data_ptr())
        ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
        ix.sync()
        del d_packed, d_starts
        res["synthetic"], spec = measure(ix, a.reps, key_bytes)
        if a.host_route:
            t0 = time.perf_counter()
            lo, hi, idx, cnt = ix.enumerate(chunk=1 << 26)
            t1 = time.perf_counter()
            hist = np.bincount(cnt, minlength=256)
            t2 = time.perf_counter()
            keepers = cnt >= 2
            kept = (lo[keepers], hi[keepers], idx[keepers], cnt[keepers])
            t3 = time.perf_counter()
            assert np.array_equal(hist.astype(np.uint64), spec)
            res["host_route"] = {"enumerate_s": round(t1 - t0, 2), "bincount_s": round(t2 - t1, 3), "filter_s": round(t3 - t2, 3), "bytes_over_pcie": int(len(cnt)) * 18, "kept": int(len(kept[0]))}
            del lo, hi, idx, cnt, kept
        res["synthetic"]["prune_2_255"] = prune_once(ix, spec, key_bytes)
        ix.close()
    if a.error_reads:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from density_reads import dense_reads
        t0 = time.perf_counter()
        flat, offs = dense_reads(a.error_reads, a.k, int(a.error_reads * 150 / 10.3), 4010, e=0.001, n_special=0)
        gen_s = time.perf_counter() - t0
        nr = len(offs) - 1
        ix = brisk_amd.BriskHip(a.k, a.m, a.b, immediate_inserts=True, part_bits=a.part_bits)
        key_bytes = 8 if 2 * a.b + ix.layout["ext_bits"] - ix.layout["part_bits"] + 2 * (a.k - a.b) + 6 <= 64 else 16
        d_bases = torch.from_numpy(flat).cuda()
        d_packed = torch.zeros((len(flat) + 15) // 16 + 4, dtype=torch.int32, device="cuda")
        d_starts = torch.from_numpy(offs.astype(np.int64)).cuda()
        sums = torch.zeros(nr, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ix.pack_ascii(d_bases.data_ptr(), len(flat), d_packed.data_ptr())
        ix.sync()
        del d_bases
        ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), nr)
        ix.sync()
        err, spec = measure(ix, a.reps, key_bytes)
        err["reads"], err["generator_s"] = nr, round(gen_s, 1)
        get = lambda: ix.get_packed(d_packed.data_ptr(), d_starts.data_ptr(), nr, sums.data_ptr())
        before = [timed(get)[0] for _ in range(a.reps + 1)][1:]
        total_before = int(sums.sum().item())
        err["prune_2_255"] = prune_once(ix, spec, key_bytes)
        after = [timed(get)[0] for _ in range(a.reps + 1)][1:]
        total_after = int(sums.sum().item())
        err["get_packed_ms_before_prune"], err["get_packed_ms_after_prune"] = stat(before), stat(after)
        err["get_packed_sum_before_after"] = [total_before, total_after]
        res["error_bearing"] = err
        ix.close()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
