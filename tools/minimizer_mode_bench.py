"""What full-width minimizers (brisk_hip_options.minimizer_mode = full) cost and give, on the device.

    python tools/minimizer_mode_bench.py [--reads 50000000] [--k 63 --m 21 --b 14] [--repeats 3] [--error-rate 0.01]

bench.py's reads (synthetic, 150 nt, 15x), error-free and again with substitutions at --error-rate, counted in both modes.  Per mode
and input, one JSON line: the whole step (device events around clear + count + sync, warmed up, the median of --repeats), the scan
and the insert from the library's own per-phase events (brisk_hip_profile_read), the entries, memory_bytes, and get_kmers_packed and
correct_packed over the first --lookup-reads reads with correct_packed's counters.  Nothing is asserted: this tool reports."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brisk_amd  # noqa: E402
from brisk_amd.exchange import suggest_part_bits  # noqa: E402


def timed(stream, fn):
    """milliseconds between two device events around fn(), which ends in a synchronise"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    out = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), out


def substitute(d_packed, n_words, rate, seed):
    """every nucleotide of the packed stream replaced by another one with probability `rate` (input preparation, not a timed path)"""
    g = torch.Generator(device=d_packed.device)
    g.manual_seed(seed)
    words = d_packed[:n_words]
    for j in range(16):
        hit = torch.rand(n_words, device=d_packed.device, generator=g) < rate
        sub = torch.randint(1, 4, (n_words,), device=d_packed.device, generator=g, dtype=torch.int32)
        words ^= torch.where(hit, sub, torch.zeros_like(sub)) << (30 - 2 * j)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--k", type=int, default=63)
    ap.add_argument("--m", type=int, default=21)
    ap.add_argument("--b", type=int, default=14)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--coverage", type=float, default=15.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--lookup-reads", type=int, default=10_000_000, help="reads of the get_kmers_packed / correct_packed leg")
    args = ap.parse_args()
    k, m, b, L, n = args.k, args.m, args.b, args.read_len, args.reads
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    n_words = (n * L + 15) // 16
    with torch.cuda.stream(stream):
        d_packed = torch.zeros(n_words + 4, dtype=torch.int32, device=dev)
        d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    stream.synchronize()
    part_bits = suggest_part_bits(b, n, L - k + 1, min_bits=22 if k <= 32 else 24, per_partition=1024 if k <= 32 else 512)
    n_look = min(args.lookup_reads, n)
    n_slots = n_look * (L - k + 1)
    for rate in (0.0, args.error_rate):
        with brisk_amd.BriskHip(k, m, b, stream=stream.cuda_stream, part_bits=2) as gen:
            gen.synth_reads(max(int(n * L / args.coverage), L + 1), 0, n, L, d_packed.data_ptr(), d_starts.data_ptr())
            gen.sync()
        if rate:
            with torch.cuda.stream(stream):
                substitute(d_packed, n_words, rate, 7)
            stream.synchronize()
        for mode in ("reference", "full"):
            with brisk_amd.BriskHip(k, m, b, stream=stream.cuda_stream, part_bits=part_bits, minimizer_mode=mode) as ix:
                def step():
                    ix.clear()
                    ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
                    ix.sync()

                step()  # warm-up: arena mapped, kernels loaded
                ix.profile_enable(True)
                ix.profile_reset()
                ms = [timed(stream, step)[0] for _ in range(args.repeats)]
                prof = {name: round(v["ms"] / args.repeats, 3) for name, v in ix.profile_read().items() if v["launches"]}
                ix.profile_enable(False)
                st = ix.stats()
                line = {"mode": mode, "error_rate": rate, "k": k, "m": m, "b": b, "reads": n, "step_ms": round(statistics.median(ms), 2), "step_ms_all": [round(x, 2) for x in ms],
                        "phases_ms": prof, "entries": st["nb_kmers"], "memory_bytes": st["memory_bytes"], "checksum": list(ix.checksum())}
                with torch.cuda.stream(stream):
                    d_slots = torch.zeros(n_slots + 8, dtype=torch.int16, device=dev)
                    d_out = torch.zeros(n_words + 4, dtype=torch.int32, device=dev)
                stream.synchronize()

                def get():
                    ix.get_kmers_packed(d_packed.data_ptr(), d_starts.data_ptr(), n_look, d_slots.data_ptr())
                    ix.sync()

                def correct():
                    st = ix.correct_packed(d_packed.data_ptr(), d_starts.data_ptr(), n_look, d_out.data_ptr(), n_words, 0, 0, 2, None)
                    ix.sync()
                    return st

                get()
                line["get_kmers_packed_ms"] = round(statistics.median(timed(stream, get)[0] for _ in range(args.repeats)), 2)
                line["get_kmers_found"] = int(((d_slots[:n_slots].to(torch.int32) & 0x100) != 0).sum().item())
                line["lookup_reads"], line["lookup_slots"] = n_look, n_slots
                correct()
                runs = [timed(stream, correct) for _ in range(args.repeats)]
                line["correct_packed_ms"] = round(statistics.median(r[0] for r in runs), 2)
                line["correct_counters"] = {key: int(v) for key, v in runs[-1][1].items()}
                del d_slots, d_out
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
