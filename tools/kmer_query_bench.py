"""Per-k-mer get against the per-read get on the bench's index: 50 M synthetic 150 bp reads at 15x coverage, k63 m21 b14
(bench.py's workload), inserted, then queried with the same reads by brisk_hip_get_packed (one sum per read) and
brisk_hip_get_kmers_packed (one uint16 per k-mer position), alternating, host clocks around synchronised calls.

Checks what the two answers must share: every slot is found (the reads were inserted), and no read's sum of counts over its slots
is below its get_packed sum (get_packed stops a read at a returned minimizer of 0: it can only drop k-mers).  Prints one JSON line.

    python tools/kmer_query_bench.py [--reads 50000000] [--reps 5] [--k 63 --m 21 --b 14]
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
    ap.add_argument("--coverage", type=float, default=15.0)
    a = ap.parse_args()
    n, L, k = a.reads, 150, a.k
    G = max(int(n * L / a.coverage), L + 1)
    dev = torch.device("cuda", 0)
    d_packed = torch.zeros((n * L + 15) // 16 + 4, dtype=torch.int32, device=dev)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    sums = torch.zeros(n, dtype=torch.int64, device=dev)
    n_slots = n * max(L - k + 1, 0)
    d_out = torch.zeros(n_slots, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()  # torch fills on its own stream, the library works on another
    ix = brisk_amd.BriskHip(a.k, a.m, a.b)
    ix.synth_reads(G, 0, n, L, d_packed.data_ptr(), d_starts.data_ptr())
    ix.sync()
    ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
    ix.sync()
    st = ix.stats()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    get_ms, kmers_ms = [], []
    for rep in range(a.reps + 1):  # the first pair warms up (allocations)
        g = timed(lambda: ix.get_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, sums.data_ptr()))
        q = timed(lambda: ix.get_kmers_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_out.data_ptr()))
        if rep:
            get_ms.append(g)
            kmers_ms.append(q)
    # checks, on the device: every slot found; per read, sum of slot counts >= get_packed's sum
    out = d_out.view(n, L - k + 1).to(torch.int32) & 0xFFFF
    all_found = bool(((out & 0x100) != 0).all().item())
    per_read = (out & 0xFF).sum(dim=1, dtype=torch.int64)
    covers = bool((per_read >= sums).all().item())
    equal_reads = int((per_read == sums).sum().item())
    del out, per_read
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"workload": "%d synthetic %d bp reads, %gx coverage, k=%d m=%d b=%d" % (n, L, a.coverage, a.k, a.m, a.b),
           "index": {"nb_kmers": st["nb_kmers"], "nb_buckets": st["nb_buckets"]}, "slots": n_slots,
           "get_packed_ms": {"median": round(med(get_ms), 2), "all": [round(x, 2) for x in get_ms]},
           "get_kmers_packed_ms": {"median": round(med(kmers_ms), 2), "all": [round(x, 2) for x in kmers_ms]},
           "ratio": round(med(kmers_ms) / med(get_ms), 3),
           "checks": {"every_slot_found": all_found, "slot_sums_cover_read_sums": covers, "reads_with_equal_sums": equal_reads}}
    ix.close()
    print(json.dumps(res))
    return 0 if all_found and covers else 1


if __name__ == "__main__":
    sys.exit(main())
