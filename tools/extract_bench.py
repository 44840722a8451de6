"""Read extraction on the bench's workload: N synthetic 150 bp reads at 15x coverage (k63 m21 b14 by default: bench.py's), resident on
the device as a packed stream and inserted, then

  1. brisk_hip_trim_packed (profile, rule, gather) against brisk_hip_read_profile_packed alone, alternating, host clocks around
     synchronised calls, the first pair a warm-up, medians: what acting on the profile costs on top of computing it;
  2. brisk_hip_extract_packed alone, on given intervals ([--start, --start + --len) of two reads in three, and every read whole),
     against a device-to-device hipMemcpyAsync (torch's contiguous copy_) that moves the same number of bytes, read plus written,
     on the same device in the same process: the copy is the yardstick;
  3. the host route the call replaces, on --host-reads reads: the profile records over PCIe, the ASCII reads sliced with numpy,
     the kept stretches uploaded and packed on the device.

Checks the gathered stream of case 2 against the input through unpack_ascii on sampled reads.  Prints one JSON line.

    python tools/extract_bench.py [--reads 50000000] [--reps 5] [--k 63 --m 21 --b 14] [--host-reads 2000000] [--solid 2]
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
    ap.add_argument("--host-reads", type=int, default=2_000_000)
    ap.add_argument("--solid", type=int, default=2)
    ap.add_argument("--start", type=int, default=7)
    ap.add_argument("--len", type=int, default=120)
    a = ap.parse_args()
    n, L = a.reads, 150
    assert a.start + a.len <= L
    G = max(int(n * L / a.coverage), L + 1)
    dev = torch.device("cuda", 0)
    n_words = (n * L + 15) // 16
    d_packed = torch.zeros(n_words + 4, dtype=torch.int32, device=dev)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_prof = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n_words + 4, dtype=torch.int32, device=dev)
    d_os = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_oi = torch.zeros(n, dtype=torch.int64, device=dev)
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
    rule = brisk_amd.select_rule("solid_run")
    # ---- 1: trim_packed against read_profile_packed alone
    kept = {}
    profile = lambda: ix.read_profile_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_prof.data_ptr(), a.solid)

    def trim():
        kept["trim"] = ix.trim_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_out.data_ptr(), n_words + 4, d_os.data_ptr(), d_oi.data_ptr(), a.solid, rule)

    prof_ms, trim_ms = [], []
    for rep in range(a.reps + 1):  # the first pair warms up (allocations)
        p, t = timed(profile), timed(trim)
        if rep:
            prof_ms.append(p)
            trim_ms.append(t)
    # ---- 2: extract_packed alone against a device-to-device copy of the same bytes
    d_iv = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    cases = {}
    for name in ("two_reads_in_three", "every_read_whole"):
        if name == "two_reads_in_three":
            keep = (torch.arange(n, device=dev) % 3) != 0
            d_iv[:, 0] = torch.where(keep, a.start, 0)
            d_iv[:, 1] = torch.where(keep, a.len, 0)
            del keep
        else:
            d_iv[:, 0] = 0
            d_iv[:, 1] = L
        torch.cuda.synchronize()

        def extract():
            kept[name] = ix.extract_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_iv.data_ptr(), d_out.data_ptr(), n_words + 4, d_os.data_ptr(), d_oi.data_ptr())

        ms = [timed(extract) for _ in range(a.reps + 1)][1:]
        n_out, n_nts = kept[name]
        # the call reads the read table (8 B a read) and the intervals (8 B) twice, the kept nucleotides (2 bits each; whole words
        # of them), out_starts and the kept reads' source positions in the gather (8 B each a kept read), and writes the output
        # words, out_starts, out_index and the source positions (8 B each a kept read)
        read_b = 2 * n * 16 + n_nts // 4 + 2 * n_out * 8
        written_b = n_nts // 4 + 3 * n_out * 8
        copy_words = (read_b + written_b) // 2 // 4  # a copy of X bytes reads X and writes X
        src = torch.zeros(copy_words, dtype=torch.int32, device=dev)
        dst = torch.empty_like(src)
        copy_ms = [timed(lambda: dst.copy_(src)) for _ in range(a.reps + 1)][1:]
        del src, dst
        torch.cuda.empty_cache()
        cases[name] = {"kept_reads": n_out, "kept_nts": n_nts, "extract_packed_ms": {"median": round(med(ms), 3), "all": rnd(ms)},
                       "bytes_read": read_b, "bytes_written": written_b, "d2d_copy_of_half_that_ms": {"median": round(med(copy_ms), 3), "all": rnd(copy_ms)},
                       "extract_over_copy": round(med(ms) / med(copy_ms), 2), "GB_per_s": round((read_b + written_b) / med(ms) / 1e6, 1)}
        if name == "two_reads_in_three":  # sampled reads of the output against the same stretch of the input
            rng = np.random.default_rng(1)
            sample = np.unique(np.concatenate([[0, n_out - 1], rng.integers(0, n_out, 2000)]))
            d_a = torch.zeros(len(sample) * a.len, dtype=torch.uint8, device=dev)
            d_b = torch.zeros(len(sample) * a.len, dtype=torch.uint8, device=dev)
            idx = d_oi[:n_out].cpu().numpy()[sample]
            torch.cuda.synchronize()
            for i, (j, r) in enumerate(zip(sample.tolist(), idx.tolist())):
                ix.unpack_ascii(d_out.data_ptr(), j * a.len, a.len, d_a.data_ptr() + i * a.len)
                ix.unpack_ascii(d_packed.data_ptr(), r * L + a.start, a.len, d_b.data_ptr() + i * a.len)
            ix.sync()
            cases[name]["sampled_reads_equal_the_input"] = bool(torch.equal(d_a, d_b)) and bool((idx % 3 != 0).all())
    del d_iv
    torch.cuda.empty_cache()
    # ---- 3: the host route on the first hn reads: records over PCIe, numpy slicing of ASCII, upload and pack
    hn = min(a.host_reads, n)
    host = {}
    if hn:
        d_ascii = torch.zeros(hn * L, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ix.unpack_ascii(d_packed.data_ptr(), 0, hn * L, d_ascii.data_ptr())
        ix.sync()
        flat = d_ascii.cpu().numpy()  # the host's copy of its reads (not timed: the host route has it)
        offs = np.arange(hn + 1, dtype=np.int64) * L
        d_up = torch.zeros(hn * L, dtype=torch.uint8, device=dev)
        d_pk = torch.zeros((hn * L + 15) // 16 + 4, dtype=torch.int32, device=dev)
        parts = {}

        def host_route():
            t0 = time.perf_counter()
            ix.read_profile_packed(d_packed.data_ptr(), d_starts.data_ptr(), hn, d_prof.data_ptr(), a.solid)
            t1 = time.perf_counter()
            rec = d_prof[:hn * 32].cpu().numpy().view(brisk_amd.READ_PROFILE_DTYPE)
            t2 = time.perf_counter()
            iv = brisk_amd.intervals_from_profile(rec, a.k, rule)
            ln = iv["len"].astype(np.int64)
            keep = ln > 0
            first = np.cumsum(ln) - ln
            total = int(ln.sum())
            src = np.repeat(offs[:-1] + iv["start"], ln) + (np.arange(total, dtype=np.int64) - np.repeat(first, ln))
            out = flat[src]
            t3 = time.perf_counter()
            d_up[:total].copy_(torch.from_numpy(out))
            torch.cuda.synchronize()
            ix.pack_ascii(d_up.data_ptr(), total, d_pk.data_ptr())
            ix.sync()
            t4 = time.perf_counter()
            parts.update(profile_ms=(t1 - t0) * 1e3, records_to_host_ms=(t2 - t1) * 1e3, numpy_slicing_ms=(t3 - t2) * 1e3, upload_and_pack_ms=(t4 - t3) * 1e3,
                         kept_reads=int(keep.sum()), kept_nts=total)

        def device_route():
            kept["host_n"] = ix.trim_packed(d_packed.data_ptr(), d_starts.data_ptr(), hn, d_out.data_ptr(), n_words + 4, d_os.data_ptr(), d_oi.data_ptr(), a.solid, rule)

        h_ms, d_ms = [], []
        for rep in range(min(a.reps, 3) + 1):
            h, d = timed(host_route), timed(device_route)
            if rep:
                h_ms.append(h)
                d_ms.append(d)
        same = bool(torch.equal(d_pk[:(parts["kept_nts"] + 15) // 16], d_out[:(parts["kept_nts"] + 15) // 16])) and kept["host_n"] == (parts["kept_reads"], parts["kept_nts"])
        host = {"reads": hn, "host_route_ms": {"median": round(med(h_ms), 2), "all": rnd(h_ms)}, "last_run_parts": {k: (round(v, 2) if isinstance(v, float) else v) for k, v in parts.items()},
                "trim_packed_same_reads_ms": {"median": round(med(d_ms), 2), "all": rnd(d_ms)}, "both_routes_give_the_same_stream": same}
    res = {"tool": "extract_bench", "config": {"reads": n, "read_len": L, "k": a.k, "m": a.m, "b": a.b, "coverage": a.coverage, "solid_min": a.solid, "reps": a.reps},
           "entries": ix.stats()["nb_kmers"],
           "read_profile_packed_ms": {"median": round(med(prof_ms), 2), "all": rnd(prof_ms)},
           "trim_packed_ms": {"median": round(med(trim_ms), 2), "all": rnd(trim_ms)},
           "trim_minus_profile_ms": round(med(trim_ms) - med(prof_ms), 2), "trim_kept": list(kept["trim"]),
           "extract_packed_alone": cases, "host_route": host}
    print(json.dumps(res))
    ix.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
