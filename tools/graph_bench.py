"""What the de Bruijn adjacency calls cost on the device (brisk_hip_adjacency / _degree_spectrum / _prune_degrees).

    python tools/graph_bench.py [--reads 50000000] [--repeats 3] [--host-reads 100000] [--out profiles/r30_graph.json]

bench.py's reads (synthetic, 150 nt, 15x) counted at k63 m21 b14 in full mode and at k31 m15 b14.  Per geometry: adjacency into a
device buffer (device events around the call, warmed up, the median of --repeats) with its three phases -- the neighbour-read kernel,
the lookups, the fold -- from the library's own per-phase events (brisk_hip_graph_phase_ms), degree_spectrum, and prune_degrees with
the isolated mask; for context, not as a bar, get_kmers_packed over (nearly) the same number of k-mer lookups taken from the 150-nt
reads: what the one-k-mer reads cost.  Then, on the index of --host-reads reads (about 1 M entries), the route that existed before:
enumerate + neighbour_strings + get_kmers + numpy on the host, wall clock.  Nothing is asserted: this tool reports."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brisk_amd  # noqa: E402
from brisk_amd.exchange import suggest_part_bits  # noqa: E402

GEOMETRIES = [(63, 21, 14, "full"), (31, 15, 14, "reference")]


def timed(stream, fn):
    """milliseconds between two device events around fn(), which ends in a synchronise"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    out = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), out


def median_of(stream, fn, repeats):
    fn()  # warm-up: scratch allocated, kernels loaded
    runs = [timed(stream, fn) for _ in range(repeats)]
    return round(statistics.median(r[0] for r in runs), 2), [round(r[0], 2) for r in runs], runs[-1][1]


def synth(k, m, b, stream, n, L, coverage, d_packed, d_starts):
    with brisk_amd.BriskHip(k, m, b, stream=stream.cuda_stream, part_bits=2) as gen:
        gen.synth_reads(max(int(n * L / coverage), L + 1), 0, n, L, d_packed.data_ptr(), d_starts.data_ptr())
        gen.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--coverage", type=float, default=15.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-reads", type=int, default=100_000, help="reads of the index the host route is measured on (100 000: about 1 M entries)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L, n = args.read_len, args.reads
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    n_words = (n * L + 15) // 16
    with torch.cuda.stream(stream):
        d_packed = torch.zeros(n_words + 4, dtype=torch.int32, device=dev)
        d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    stream.synchronize()
    result = {"reads": n, "read_len": L, "coverage": args.coverage, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "geometries": []}
    for k, m, b, mode in GEOMETRIES:
        synth(k, m, b, stream, n, L, args.coverage, d_packed, d_starts)
        part_bits = suggest_part_bits(b, n, L - k + 1, min_bits=22 if k <= 32 else 24, per_partition=1024 if k <= 32 else 512)
        with brisk_amd.BriskHip(k, m, b, stream=stream.cuda_stream, part_bits=part_bits, minimizer_mode=mode) as ix:
            ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
            ix.sync()
            entries = ix.stats()["nb_kmers"]
            with torch.cuda.stream(stream):
                d_adj = torch.zeros(entries + 8, dtype=torch.uint8, device=dev)
            stream.synchronize()
            ix.profile_enable(True)
            line = {"k": k, "m": m, "b": b, "minimizer_mode": mode, "part_bits": part_bits, "entries": entries, "lookups": 8 * entries}
            line["adjacency_ms"], line["adjacency_ms_all"], _ = median_of(stream, lambda: ix.adjacency_device(d_adj.data_ptr(), entries, 0), args.repeats)
            line["adjacency_phases_ms"] = {name: round(v, 2) for name, v in ix.graph_phase_ms().items()}
            line["degree_spectrum_ms"], line["degree_spectrum_ms_all"], sp = median_of(stream, lambda: ix.degree_spectrum(0), args.repeats)
            line["figures"] = brisk_amd.graph_figures(sp)
            ix.profile_enable(False)
            line["prune_isolated_ms"], line["prune_isolated_ms_all"], _ = median_of(stream, lambda: ix.prune_degrees([(0, 0)]), args.repeats)
            line["entries_after_prune"] = ix.stats()["nb_kmers"]
            del d_adj
            # context: the same number of lookups as k-mers of 150-nt reads
            n_look = min(n, max(1, 8 * entries // (L - k + 1)))
            n_slots = n_look * (L - k + 1)
            with torch.cuda.stream(stream):
                d_slots = torch.zeros(n_slots + 8, dtype=torch.int16, device=dev)
            stream.synchronize()

            def get():
                ix.get_kmers_packed(d_packed.data_ptr(), d_starts.data_ptr(), n_look, d_slots.data_ptr())
                ix.sync()

            line["get_kmers_packed_ms"], line["get_kmers_packed_ms_all"], _ = median_of(stream, get, args.repeats)
            line["get_kmers_packed_reads"], line["get_kmers_packed_lookups"] = n_look, n_slots
            line["ns_per_lookup"] = {"adjacency": round(line["adjacency_ms"] * 1e6 / (8 * entries), 3), "get_kmers_packed": round(line["get_kmers_packed_ms"] * 1e6 / n_slots, 3)}
            del d_slots
        result["geometries"].append(line)
        print(json.dumps(line), flush=True)
    # the host route that existed before, on about 1 M entries
    k, m, b, mode = GEOMETRIES[0]
    nh = min(args.host_reads, n)
    synth(k, m, b, stream, nh, L, args.coverage, d_packed, d_starts)
    with brisk_amd.BriskHip(k, m, b, stream=stream.cuda_stream, minimizer_mode=mode) as ix:
        ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), nh)
        ix.sync()
        t0 = time.perf_counter()
        lo, hi, idx, cnt = ix.enumerate()
        t1 = time.perf_counter()
        strings = brisk_amd.neighbour_strings(lo, hi, k)
        t2 = time.perf_counter()
        counts, found, base = ix.get_kmers(strings)
        t3 = time.perf_counter()
        adj = brisk_amd.adjacency_from_slots(counts, found, 0)
        sp_host = brisk_amd.degree_spectrum_from_adjacency(adj, cnt, 0)
        t4 = time.perf_counter()
        with torch.cuda.stream(stream):
            d_adj = torch.zeros(len(lo) + 8, dtype=torch.uint8, device=dev)
        stream.synchronize()
        dev_ms, dev_all, _ = median_of(stream, lambda: ix.adjacency_device(d_adj.data_ptr(), len(lo), 0), args.repeats)
        same = bool(np.array_equal(d_adj[:len(lo)].cpu().numpy(), adj)) and bool(np.array_equal(ix.degree_spectrum(0), sp_host))
        result["host_route"] = {"k": k, "m": m, "b": b, "minimizer_mode": mode, "reads": nh, "entries": int(len(lo)),
                                "enumerate_s": round(t1 - t0, 3), "neighbour_strings_s": round(t2 - t1, 3), "get_kmers_s": round(t3 - t2, 3), "numpy_fold_s": round(t4 - t3, 3),
                                "total_s": round(t4 - t0, 3), "device_adjacency_ms": dev_ms, "device_adjacency_ms_all": dev_all, "same_bytes": same}
        print(json.dumps(result["host_route"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
