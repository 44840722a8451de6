"""Per-read profiles against the per-k-mer get they reduce, on the bench's index: N synthetic 150 bp reads at 15x coverage (k63 m21
b14 by default: bench.py's workload), inserted, then

  1. device-resident reads: brisk_hip_read_profile_packed against brisk_hip_get_kmers_packed, alternating, host clocks around
     synchronised calls, the first pair a warm-up, medians; the reduction kernels' own time from the library's profile slots
     (a separate pass with profiling on), against the time the profiled run's k_spectrum-rate would need for slots x 2 bytes;
  2. host reads (--host-reads M of them): read_profile against get_kmers followed by the vectorisable part of the reduction in
     numpy (n_present, n_solid, sum, min, max per read: one reduceat each) -- the route the profile replaces;
  3. device memory: what each route holds at its peak beyond the reads and the index (free memory sampled by the caller around
     the calls, the caller's slot array included for get_kmers_packed).

Checks that the records equal a reduction of get_kmers_packed's slots done with torch on the device (n_present, n_solid, sum, min,
max, run over reads of equal length).  Prints one JSON line.

    python tools/read_profile_bench.py [--reads 50000000] [--reps 5] [--k 63 --m 21 --b 14] [--host-reads 1000000] [--solid 2]
"""
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=63)
    ap.add_argument("--m", type=int, default=21)
    ap.add_argument("--b", type=int, default=14)
    ap.add_argument("--part-bits", type=int, default=0)
    ap.add_argument("--coverage", type=float, default=15.0)
    ap.add_argument("--host-reads", type=int, default=1_000_000)
    ap.add_argument("--solid", type=int, default=2)
    a = ap.parse_args()
    n, L, k = a.reads, 150, a.k
    per = L - k + 1
    G = max(int(n * L / a.coverage), L + 1)
    dev = torch.device("cuda", 0)
    d_packed = torch.zeros((n * L + 15) // 16 + 4, dtype=torch.int32, device=dev)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_prof = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    n_slots = n * per
    torch.cuda.synchronize()  # torch fills on its own stream, the library works on another
    ix = brisk_amd.BriskHip(a.k, a.m, a.b, part_bits=a.part_bits)
    ix.synth_reads(G, 0, n, L, d_packed.data_ptr(), d_starts.data_ptr())
    ix.sync()
    ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
    ix.sync()
    st = ix.stats()
    free = lambda: torch.cuda.mem_get_info(dev)[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    med = lambda v: sorted(v)[len(v) // 2]
    profile = lambda: ix.read_profile_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_prof.data_ptr(), a.solid)
    # ---- 3 (first: the library's scratch has not grown yet; it is kept from call to call, so free memory after a call shows
    # what the call needed).  get_kmers_packed first: the scan and probe scratch is shared, what the profile adds comes on top.
    free_0 = free()
    d_out = torch.zeros(max(n_slots, 1), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    kmers = lambda: ix.get_kmers_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_out.data_ptr())
    kmers()
    torch.cuda.synchronize()
    free_1 = free()
    profile()
    torch.cuda.synchronize()
    profile_extra = free_1 - free()
    kmers_scratch = free_0 - free_1 - d_out.numel() * 2
    # ---- 1
    prof_ms, kmers_ms = [], []
    for rep in range(a.reps + 1):  # the first pair warms up (allocations)
        q = timed(kmers)
        p = timed(profile)
        if rep:
            kmers_ms.append(q)
            prof_ms.append(p)
    ix.profile_enable(True)
    ix.profile_reset()
    profile()
    ix.count_spectrum()
    slots_prof = {name: v for name, v in ix.profile_read().items() if v["launches"]}
    ix.profile_enable(False)
    # k_spectrum has no profile slot: host clock around the synchronised call, a pass over the arena's count bytes
    spec_ms = med([timed(ix.count_spectrum) for _ in range(a.reps)])
    reduce_ms = slots_prof.get("k_profile_reads", {}).get("ms", 0.0) + slots_prof.get("k_profile_segments_and_fold", {}).get("ms", 0.0)
    # ---- the records against the slots, reduced on the device with torch
    out = (d_out.view(n, per).to(torch.int32) & 0xFFFF) if n_slots else None
    rec = d_prof.cpu().numpy().view(brisk_amd.READ_PROFILE_DTYPE)
    checks = {}
    if out is not None:
        present = (out & 0x100) != 0
        cnt = out & 0xFF
        solid = present & (cnt >= a.solid)
        checks["n_kmers"] = bool((rec["n_kmers"] == per).all())
        checks["n_present"] = bool(np.array_equal(rec["n_present"], present.sum(dim=1).cpu().numpy()))
        checks["n_solid"] = bool(np.array_equal(rec["n_solid"], solid.sum(dim=1).cpu().numpy()))
        checks["sum"] = bool(np.array_equal(rec["sum"], torch.where(present, cnt, 0).sum(dim=1, dtype=torch.int64).cpu().numpy().astype(np.uint64)))
        checks["max_present"] = bool(np.array_equal(rec["max_present"], torch.where(present, cnt, 0).amax(dim=1).cpu().numpy()))
        nm = min(n, 5_000_000)  # (a sort of every slot would need ten times the slots' memory)
        checks["median_first_reads"] = bool(np.array_equal(rec["median"][:nm], torch.where(present[:nm], cnt[:nm], 0).sort(dim=1).values[:, (per - 1) // 2].cpu().numpy()))
        full = solid.all(dim=1).cpu().numpy()
        checks["run_of_fully_solid_reads"] = bool(((rec["run_start"][full] == 0) & (rec["run_len"][full] == per)).all())
        checks["fully_solid_reads"] = int(full.sum())
        del present, cnt, solid, out
    del d_out
    torch.cuda.empty_cache()
    # ---- 2: host reads
    host = {}
    hn = min(a.host_reads, n)
    if hn:
        codes = np.frombuffer(b"ACTG", np.uint8)  # the packed stream's code -> nucleotide (A0 C1 T2 G3)
        words = d_packed[: (hn * L + 15) // 16].cpu().numpy().view(np.uint32)
        shifts = np.arange(30, -2, -2, dtype=np.uint32)
        flat = codes[((words[:, None] >> shifts[None, :]) & 3).reshape(-1)[: hn * L]]
        offs = np.arange(hn + 1, dtype=np.uint64) * L
        base = brisk_amd.kmer_slots(offs, k)
        total = int(base[-1])
        slots = np.zeros(max(total, 1), np.uint16)
        recs = np.zeros(hn, brisk_amd.READ_PROFILE_DTYPE)
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(16)  # numpy releases the interpreter lock inside its loops: 16 threads' worth
        cuts = [hn * t // 16 for t in range(17)]

        def reduce_part(t):
            r0, r1 = cuts[t], cuts[t + 1]
            if r0 == r1:
                return tuple(np.zeros(0, np.uint64) for _ in range(5))
            s = slots[int(base[r0]):int(base[r1])]
            c, f = (s & 0xff), (s & 0x100) != 0
            at = (base[r0:r1] - base[r0]).astype(np.int64)
            return (np.add.reduceat(f.astype(np.uint32), at), np.add.reduceat((f & (c >= a.solid)).astype(np.uint32), at),
                    np.add.reduceat(np.where(f, c, 0).astype(np.uint64), at), np.maximum.reduceat(np.where(f, c, 0), at),
                    np.minimum.reduceat(np.where(f, c, 255), at))

        def old_route():
            ix._chk(ix.L.brisk_hip_get_kmers(ix.h, flat, offs, hn, slots, total))
            parts = list(pool.map(reduce_part, range(16)))
            return tuple(np.concatenate([p[i] for p in parts]) for i in range(5))

        new_route = lambda: ix._chk(ix.L.brisk_hip_read_profile_reads(ix.h, flat, offs, hn, a.solid, recs))
        old_ms, new_ms, get_only_ms = [], [], []
        for rep in range(min(a.reps, 3) + 1):
            o = timed(old_route)
            g = timed(lambda: ix._chk(ix.L.brisk_hip_get_kmers(ix.h, flat, offs, hn, slots, total)))
            p = timed(new_route)
            if rep:
                old_ms.append(o)
                get_only_ms.append(g)
                new_ms.append(p)
        res_old = old_route()
        host = {"reads": hn, "read_profile_ms": round(med(new_ms), 2), "get_kmers_then_numpy_ms": round(med(old_ms), 2), "of_which_get_kmers_ms": round(med(get_only_ms), 2),
                "bytes_back_read_profile": hn * 32, "bytes_back_get_kmers": total * 2,
                "agree": bool(np.array_equal(res_old[0], recs["n_present"]) and np.array_equal(res_old[1], recs["n_solid"]) and np.array_equal(res_old[2], recs["sum"]))}
    mem = ix.memory_info()
    ideal_ms = None
    if spec_ms > 0:
        spectrum_gbs = st["nb_kmers"] / spec_ms / 1e6  # the spectrum reads one count byte an entry (and the directory)
        ideal_ms = n_slots * 2 / (spectrum_gbs * 1e6)
    res = {"workload": "%d synthetic %d bp reads, %gx coverage, k=%d m=%d b=%d" % (n, L, a.coverage, a.k, a.m, a.b),
           "index": {"nb_kmers": st["nb_kmers"], "nb_buckets": st["nb_buckets"]}, "slots": n_slots, "solid_min": a.solid,
           "get_kmers_packed_ms": {"median": round(med(kmers_ms), 2), "all": [round(x, 2) for x in kmers_ms]},
           "read_profile_packed_ms": {"median": round(med(prof_ms), 2), "all": [round(x, 2) for x in prof_ms]},
           "ratio": round(med(prof_ms) / med(kmers_ms), 3),
           "profile_slots_ms": {name: round(v["ms"], 3) for name, v in slots_prof.items()},
           "reduction_kernels_ms": round(reduce_ms, 3), "count_spectrum_call_ms": round(spec_ms, 3),
           "slots_x2_bytes_at_the_spectrum_call_rate_ms": None if ideal_ms is None else round(ideal_ms, 3),
           "device_memory": {"scan_and_probe_scratch_bytes_both_routes": int(kmers_scratch), "read_profile_packed_adds_bytes": int(profile_extra),
                             "read_profile_packed_records_bytes": n * 32, "get_kmers_packed_caller_slot_array_bytes": n_slots * 2, "arena_mapped": mem["arena_mapped"]},
           "host_route": host, "checks": checks}
    ix.close()
    print(json.dumps(res))
    ok = all(v for key, v in checks.items() if key != "fully_solid_reads") and (not host or host["agree"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
