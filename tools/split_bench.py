"""Read splitting on the bench's workload: N synthetic 150 bp reads at 15x coverage (k63 m21 b14 by default: bench.py's), resident on
the device as a packed stream and inserted; once as they are ("clean") and once with 1 % of the nucleotides substituted before the
count ("errors": the k-mers over an error are seen once, so they are weak at --solid 2).  Per set, host clocks around synchronised
calls, the first repetition a warm-up, medians:

  1. brisk_hip_split_packed (lookups, run passes, gather) and brisk_hip_trim_packed over the same reads, alternating;
  2. the run passes alone: brisk_hip_solid_runs over the slots brisk_hip_get_kmers_packed left on the device;
  3. the gather alone: brisk_hip_extract_fragments_packed over the table split_packed wrote;
  4. brisk_hip_trim_packed of another build (--yardstick-root DIR, a built checkout of another commit: the parent's), in a process
     of its own (this tool with --trim-only, importing that checkout's package and library), on the same seeded reads;
  5. what each keeps: the share of the input's nucleotides and of its k-mers in split's fragments and in trim's intervals.

Prints one JSON line and, with --out, writes it there.

    python tools/split_bench.py [--reads 50000000] [--reps 5] [--k 63 --m 21 --b 14] [--solid 2] [--yardstick-root DIR] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.environ.get("BRISK_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # (the yardstick process: another checkout's package)
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import brisk_amd  # noqa: E402

L = 150
med = lambda v: sorted(v)[len(v) // 2]
figures = lambda v: {"median": round(med(v), 2), "all": [round(x, 2) for x in v]}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def substitute(d_packed, n_words, rate, seed):
    """every nucleotide of the first n_words words replaced by another one with probability `rate`, on the device, seeded"""
    gen = torch.Generator(device=d_packed.device)
    gen.manual_seed(seed)
    step = 1 << 25
    for w0 in range(0, n_words, step):
        w1 = min(w0 + step, n_words)
        mask = torch.zeros(w1 - w0, dtype=torch.int64, device=d_packed.device)
        for j in range(16):
            hit = torch.rand(w1 - w0, device=d_packed.device, generator=gen) < rate
            code = torch.randint(1, 4, (w1 - w0,), device=d_packed.device, generator=gen, dtype=torch.int64)
            mask |= torch.where(hit, code << (30 - 2 * j), torch.zeros_like(code))
        mask = torch.where(mask >= (1 << 31), mask - (1 << 32), mask).to(torch.int32)
        d_packed[w0:w1] ^= mask
    torch.cuda.synchronize()


def reads_and_index(a, errors):
    n = a.reads
    G = max(int(n * L / a.coverage), L + 1)
    dev = torch.device("cuda", 0)
    n_words = (n * L + 15) // 16
    d_packed = torch.zeros(n_words + 4, dtype=torch.int32, device=dev)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # torch fills on its own stream, the library works on another
    ix = brisk_amd.BriskHip(a.k, a.m, a.b, part_bits=a.part_bits)
    ix.synth_reads(G, 0, n, L, d_packed.data_ptr(), d_starts.data_ptr())
    ix.sync()
    if errors:
        substitute(d_packed, n * L // 16, a.error_rate, 26)
    ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
    ix.sync()
    return ix, d_packed, d_starts, n_words


def trim_only(a):
    """trim_packed alone, per set: what the yardstick process prints"""
    out = {}
    for name in a.sets.split(","):
        ix, d_packed, d_starts, n_words = reads_and_index(a, name == "errors")
        n = a.reads
        d_out = torch.zeros(n_words + 4, dtype=torch.int32, device=d_packed.device)
        d_os = torch.zeros(n + 1, dtype=torch.int64, device=d_packed.device)
        torch.cuda.synchronize()
        kept = {}

        def trim():
            kept["trim"] = ix.trim_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_out.data_ptr(), n_words + 4, d_os.data_ptr(), None, a.solid)

        ms = [timed(trim) for _ in range(a.reps + 1)][1:]
        out[name] = {"trim_packed_ms": figures(ms), "kept": list(kept["trim"]), "checksum": list(ix.checksum())}
        ix.close()
        del d_packed, d_starts, d_out, d_os
        torch.cuda.empty_cache()
    return out


def measure(a, name):
    ix, d_packed, d_starts, n_words = reads_and_index(a, name == "errors")
    n, k, dev = a.reads, a.k, d_packed.device
    P, S = d_packed.data_ptr(), d_starts.data_ptr()
    d_ask = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    st = ix.split_packed(P, S, n, 0, 0, d_ask.data_ptr(), 0, 0, a.solid, a.min_len, raise_on_capacity=False)  # the counters: a call without room fills them
    st.pop("rc", None)
    nf, need = st["n_fragments"], (st["n_nts_out"] + 15) // 16 + 2
    d_out = torch.zeros(max(need, n_words + 4), dtype=torch.int32, device=dev)
    d_os = torch.zeros(max(nf, n) + 1, dtype=torch.int64, device=dev)
    d_frags = torch.zeros(max(nf, 1) * 2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    kept = {}

    def split():
        kept["split"] = ix.split_packed(P, S, n, d_out.data_ptr(), need, d_os.data_ptr(), d_frags.data_ptr(), nf, a.solid, a.min_len)

    def trim():
        kept["trim"] = ix.trim_packed(P, S, n, d_out.data_ptr(), n_words + 4, d_os.data_ptr(), None, a.solid)

    split_ms, trim_ms = [], []
    for rep in range(a.reps + 1):  # the first pair warms up (allocations)
        s, t = timed(split), timed(trim)
        if rep:
            split_ms.append(s)
            trim_ms.append(t)
    assert kept["split"] == st
    timed(split)  # d_frags and d_out hold split's again
    # the gather alone, over split's table, into a second stream
    d_out2 = torch.zeros(need, dtype=torch.int32, device=dev)
    d_os2 = torch.zeros(nf + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def gather():
        kept["gather"] = ix.extract_fragments_packed(P, S, n, d_frags.data_ptr(), nf, d_out2.data_ptr(), need, d_os2.data_ptr())

    gather_ms = [timed(gather) for _ in range(a.reps + 1)][1:]
    same_stream = bool(torch.equal(d_out2[:need], d_out[:need])) and bool(torch.equal(d_os2, d_os[:nf + 1])) and kept["gather"] == st["n_nts_out"]
    del d_out2, d_os2
    # the run passes alone, over the slots of the whole call
    d_slots = torch.zeros(st["n_slots"] + 8, dtype=torch.int16, device=dev)
    d_frags2 = torch.zeros(max(nf, 1) * 2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    lookups_ms = [timed(lambda: ix.get_kmers_packed(P, S, n, d_slots.data_ptr())) for _ in range(a.reps + 1)][1:]

    def runs():
        kept["runs"] = ix.solid_runs(d_slots.data_ptr(), S, n, d_frags2.data_ptr(), nf, a.solid, a.min_len)

    runs_ms = [timed(runs) for _ in range(a.reps + 1)][1:]
    same_table = bool(torch.equal(d_frags2, d_frags)) and kept["runs"] == st
    n_out, n_nts = kept["trim"]
    res = {"stats": st, "split_packed_ms": figures(split_ms), "trim_packed_ms": figures(trim_ms), "split_minus_trim_ms": round(med(split_ms) - med(trim_ms), 2),
           "get_kmers_packed_ms": figures(lookups_ms), "run_passes_alone_ms": figures(runs_ms), "gather_alone_ms": figures(gather_ms),
           "gather_alone_gives_the_same_stream": same_stream, "run_passes_alone_give_the_same_table": same_table,
           "trim_kept": [n_out, n_nts],
           "share_of_nucleotides": {"split": round(st["n_nts_out"] / st["n_nts_in"], 4), "solid_run": round(n_nts / st["n_nts_in"], 4)},
           "share_of_kmers": {"split": round((st["n_nts_out"] - nf * (k - 1)) / st["n_slots"], 4), "solid_run": round((n_nts - n_out * (k - 1)) / st["n_slots"], 4),
                              "solid": round(st["n_solid"] / st["n_slots"], 4)},
           "checksum": list(ix.checksum())}
    ix.close()
    return res


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
    ap.add_argument("--min-len", type=int, default=0)
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--sets", default="clean,errors")
    ap.add_argument("--yardstick-root", default="")
    ap.add_argument("--trim-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.trim_only:
        print(json.dumps(trim_only(a)))
        return 0
    yardstick = {}
    if a.yardstick_root:  # first, while this process holds nothing on the device
        args = [sys.executable, os.path.abspath(__file__), "--trim-only"] + [x for x in sys.argv[1:] if x != "--trim-only"]
        p = subprocess.run(args, env=dict(os.environ, BRISK_BENCH_ROOT=os.path.abspath(a.yardstick_root)), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        yardstick = json.loads(p.stdout.strip().splitlines()[-1])
    res = {"tool": "split_bench",
           "config": {"reads": a.reads, "read_len": L, "k": a.k, "m": a.m, "b": a.b, "coverage": a.coverage, "solid_min": a.solid, "min_len": a.min_len, "error_rate": a.error_rate,
                      "reps": a.reps, "yardstick": bool(a.yardstick_root)},
           "sets": {name: measure(a, name) for name in a.sets.split(",")}, "yardstick_process": yardstick}
    for name, y in yardstick.items():  # the same reads and the same index in both processes
        res["sets"][name]["yardstick_saw_the_same_index_and_kept_the_same"] = y["checksum"] == res["sets"][name]["checksum"] and y["kept"] == res["sets"][name]["trim_kept"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
