"""Spectral read correction on the bench's workload: N synthetic 150 bp reads at 15x coverage (k63 m21 b14 by default: bench.py's),
resident on the device as a packed stream, with 1 % of the nucleotides substituted before the count (the k-mers over an error are
seen once, so they are weak at --solid 2) and a copy of the reads as they were: the truth.  Host clocks around synchronised calls,
the first repetition a warm-up, medians:

  1. brisk_hip_correct_packed, and brisk_hip_split_packed and brisk_hip_get_kmers_packed over the same reads, alternating;
  2. the stages alone, each over the whole call's tables: slots (get_kmers_packed), sites (weak_sites), windows
     (candidate_windows), candidate lookups (get_kmers_packed over the candidate stream), decide (decide_sites), apply
     (apply_corrections) -- and whether they give the composed call's table and stream;
  3. against the truth: the share of the planted substitutions that the output has restored, and the share of the corrections
     that disagree with the truth;
  4. the solid slots before and after (the corrected stream looked up against the same index).

Prints one JSON line and, with --out, writes it there.

    python tools/correct_bench.py [--reads 50000000] [--reps 5] [--k 63 --m 21 --b 14] [--solid 2] [--min-cover 0] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import brisk_amd  # noqa: E402
from split_bench import L, figures, med, substitute, timed  # noqa: E402


def differing(a, b, also=None):
    """nucleotides at which two packed streams differ (and, with `also`, at which a third pair differs too / does not): chunked, on the device"""
    n_both = n_only = 0
    step = 1 << 26
    m = 0x5555555555555555
    for w0 in range(0, len(a), step):
        x = (a[w0:w0 + step] ^ b[w0:w0 + step]).to(torch.int64) & 0xffffffff
        x = (x | (x >> 1)) & 0x55555555  # one bit a nucleotide that differs
        if also is None:
            n_both += int(torch.sum(_popcount(x, m)))
            continue
        y = (also[0][w0:w0 + step] ^ also[1][w0:w0 + step]).to(torch.int64) & 0xffffffff
        y = (y | (y >> 1)) & 0x55555555
        n_both += int(torch.sum(_popcount(x & y, m)))
        n_only += int(torch.sum(_popcount(x & ~y, m)))
    return n_both if also is None else (n_both, n_only)


def _popcount(x, m):
    x = x - ((x >> 1) & m)
    x = (x & 0x3333333333333333) + ((x >> 2) & 0x3333333333333333)
    x = (x + (x >> 4)) & 0x0f0f0f0f0f0f0f0f
    return (x * 0x0101010101010101) >> 56


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
    ap.add_argument("--min-cover", type=int, default=0)
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, k = a.reads, a.k
    G = max(int(n * L / a.coverage), L + 1)
    dev = torch.device("cuda", 0)
    n_words = (n * L + 15) // 16
    d_packed = torch.zeros(n_words + 4, dtype=torch.int32, device=dev)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # torch fills on its own stream, the library works on another
    ix = brisk_amd.BriskHip(a.k, a.m, a.b, part_bits=a.part_bits)
    ix.synth_reads(G, 0, n, L, d_packed.data_ptr(), d_starts.data_ptr())
    ix.sync()
    d_truth = d_packed.clone()
    substitute(d_packed, n * L // 16, a.error_rate, 26)
    ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
    ix.sync()
    P, S = d_packed.data_ptr(), d_starts.data_ptr()
    st = ix.correct_packed(P, S, n, 0, 0, 0, 0, a.solid, a.min_cover)  # the counters first: no outputs, nothing refused
    nc, ns, need = st["n_corrected"], st["n_sites"], n_words + 2
    d_out = torch.zeros(need + 2, dtype=torch.int32, device=dev)
    d_corr = torch.zeros(max(nc, 1) * 2, dtype=torch.int64, device=dev)
    ask = ix.split_packed(P, S, n, 0, 0, torch.zeros(2, dtype=torch.int64, device=dev).data_ptr(), 0, 0, a.solid, 0, raise_on_capacity=False)
    nf, split_need = ask["n_fragments"], (ask["n_nts_out"] + 15) // 16 + 2
    d_sp = torch.zeros(split_need, dtype=torch.int32, device=dev)
    d_sps = torch.zeros(nf + 1, dtype=torch.int64, device=dev)
    d_slots = torch.zeros(st["n_slots"] + 8, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    kept = {}

    def correct():
        kept["correct"] = ix.correct_packed(P, S, n, d_out.data_ptr(), need, d_corr.data_ptr(), nc, a.solid, a.min_cover)

    def split():
        ix.split_packed(P, S, n, d_sp.data_ptr(), split_need, d_sps.data_ptr(), 0, nf, a.solid, 0)

    def lookups():
        ix.get_kmers_packed(P, S, n, d_slots.data_ptr())

    correct_ms, split_ms, lookups_ms = [], [], []
    for rep in range(a.reps + 1):  # the first round warms up (allocations)
        c, s, g = timed(correct), timed(split), timed(lookups)
        if rep:
            correct_ms.append(c)
            split_ms.append(s)
            lookups_ms.append(g)
    assert kept["correct"] == st
    del d_sp, d_sps
    # against the truth
    planted = differing(d_packed[:n_words], d_truth[:n_words])
    wrong, restored = differing(d_out[:n_words], d_packed[:n_words], also=(d_out[:n_words], d_truth[:n_words]))  # changed, and now unlike / like the truth
    left = differing(d_out[:n_words], d_truth[:n_words])
    # the stages alone (d_slots holds the whole call's slots)
    d_sites = torch.zeros(max(ns, 1) * 2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def sites():
        kept["sites"] = ix.weak_sites(d_slots.data_ptr(), S, n, d_sites.data_ptr(), ns, a.solid, a.min_cover)

    sites_ms = [timed(sites) for _ in range(a.reps + 1)][1:]
    cand_nts = 3 * (int(kept["sites"]["n_sites"]) * (k - 1)) + 3 * _cover_sum(d_sites, ns)
    cand_words = (cand_nts + 15) // 16 + 2
    d_cand = torch.zeros(cand_words, dtype=torch.int32, device=dev)
    d_cst = torch.zeros(3 * ns + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def windows():
        kept["windows"] = ix.candidate_windows(P, S, n, d_sites.data_ptr(), ns, d_cand.data_ptr(), cand_words, d_cst.data_ptr())

    windows_ms = [timed(windows) for _ in range(a.reps + 1)][1:]
    assert kept["windows"] == cand_nts
    d_cslots = torch.zeros(cand_nts - 3 * ns * (k - 1) + 8, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    cand_lookups_ms = [timed(lambda: ix.get_kmers_packed(d_cand.data_ptr(), d_cst.data_ptr(), 3 * ns, d_cslots.data_ptr())) for _ in range(a.reps + 1)][1:]
    d_corr2 = torch.zeros(max(nc, 1) * 2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def decide():
        kept["decide"] = ix.decide_sites(d_cslots.data_ptr(), d_sites.data_ptr(), ns, P, S, n, d_corr2.data_ptr(), nc, a.solid)

    decide_ms = [timed(decide) for _ in range(a.reps + 1)][1:]
    same_table = bool(torch.equal(d_corr2, d_corr)) and all(kept["decide"][f] == st[f] for f in ("n_sites", "n_corrected", "n_ambiguous", "n_unresolved"))
    del d_cand, d_cst, d_cslots
    d_out2 = torch.zeros(need + 2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    apply_ms = [timed(lambda: ix.apply_corrections(P, S, n, d_corr2.data_ptr(), nc, d_out2.data_ptr(), need)) for _ in range(a.reps + 1)][1:]
    same_stream = bool(torch.equal(d_out2[:need], d_out[:need]))
    after = ix.correct_packed(d_out.data_ptr(), S, n, 0, 0, 0, 0, a.solid, a.min_cover)  # the corrected stream against the same index
    res = {"tool": "correct_bench",
           "config": {"reads": n, "read_len": L, "k": a.k, "m": a.m, "b": a.b, "coverage": a.coverage, "solid_min": a.solid, "min_cover": a.min_cover or a.k,
                      "error_rate": a.error_rate, "reps": a.reps},
           "stats": st, "correct_packed_ms": figures(correct_ms), "split_packed_ms": figures(split_ms), "get_kmers_packed_ms": figures(lookups_ms),
           "correct_over_get_kmers": round(med(correct_ms) / med(lookups_ms), 3), "correct_over_split": round(med(correct_ms) / med(split_ms), 3),
           "stages_alone_ms": {"slots": figures(lookups_ms), "sites": figures(sites_ms), "windows": figures(windows_ms), "candidate_lookups": figures(cand_lookups_ms),
                               "decide": figures(decide_ms), "apply": figures(apply_ms)},
           "candidate_stream": {"reads": 3 * ns, "nucleotides": cand_nts, "slots": cand_nts - 3 * ns * (k - 1)},
           "stages_alone_give_the_same_table": same_table, "stages_alone_give_the_same_stream": same_stream,
           "truth": {"planted": planted, "restored": restored, "share_restored": round(restored / max(planted, 1), 4), "corrections": nc,
                     "corrections_that_disagree": wrong, "share_that_disagree": round(wrong / max(nc, 1), 6), "substitutions_left": left},
           "solid_slots": {"slots": st["n_slots"], "before": st["n_slots"] - st["n_weak"], "after": after["n_slots"] - after["n_weak"],
                           "share_before": round(1 - st["n_weak"] / st["n_slots"], 4), "share_after": round(1 - after["n_weak"] / after["n_slots"], 4)},
           "stats_of_the_corrected_stream": after}
    ix.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


def _cover_sum(d_sites, ns):
    """the sum of the covers of a site table on the device (rows of two int64: read; pos | cover << 32)"""
    return int(torch.sum(d_sites[1:2 * ns:2] >> 32)) if ns else 0


if __name__ == "__main__":
    sys.exit(main())
