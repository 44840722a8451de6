"""Saturating counts (brisk_hip_options.count_mode): what the mode costs, and that the default path pays nothing for it.

    python tools/saturate_bench.py [--parent-lib libbrisk_hip_parent.so] [--procs 5] [--steps 3] [--out profiles/r10_saturate.json]

Jobs: bench.py's headline (50 M synthetic 150 bp reads, 15x, k63 m21 b14) and the 20 M-read k31 m15 b14 job, partitions by bench.py's
rule.  One measurement is one FRESH process (`--one`): the reads are generated on the device, one warm-up job, then --steps jobs,
each brisk_hip_clear + brisk_hip_insert_packed + brisk_hip_sync under the host clock; the process reports its median.
  default path   --parent-lib names a build of the parent commit next to the library (brisk_amd/<name>, chosen through
                 BRISK_HIP_LIB): parent and this build in default mode in alternating processes, --procs each.  Condition: this
                 build's median is no worse than the parent's median by more than the parent's own max - min spread.
  the mode       this build with count_mode = saturate, --procs processes, against its default mode above
  where it matters  a 100 kbp genome at 450x (300 k reads): spectrum and prune(2, 255) in both modes, in this process
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JOBS = {"k63_m21_b14_50M": dict(k=63, m=21, b=14, reads=50_000_000), "k31_m15_b14_20M": dict(k=31, m=15, b=14, reads=20_000_000)}
L, COVERAGE = 150, 15.0


def med(v):
    return sorted(v)[len(v) // 2]


def one(a):
    """a fresh process' measurement: one JSON line"""
    import torch

    import brisk_amd
    from brisk_amd.exchange import suggest_part_bits
    k, m, b, n = a.k, a.m, a.b, a.reads
    G = max(int(n * L / COVERAGE), L + 1)
    d_packed = torch.zeros((n * L + 15) // 16 + 4, dtype=torch.int32, device="cuda")
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gen = brisk_amd.BriskHip(k, m, b, part_bits=2)
    gen.synth_reads(G, 0, n, L, d_packed.data_ptr(), d_starts.data_ptr())
    gen.sync()
    gen.close()
    part_bits = suggest_part_bits(b, n, L - k + 1, min_bits=22 if k <= 32 else 24, per_partition=1024 if k <= 32 else 512)
    kw = {"count_mode": "saturate"} if a.mode == "saturate" else {}  # (a parent build is never asked for the field)
    ix = brisk_amd.BriskHip(k, m, b, part_bits=part_bits, **kw)
    times = []
    for step in range(a.steps + 1):  # the first job warms up (code objects, the arena's mappings)
        ix.clear()
        ix.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
        ix.sync()
        dt = (time.perf_counter() - t0) * 1e3
        if step:
            times.append(round(dt, 3))
    ck = ix.checksum()
    print(json.dumps({"lib": os.environ.get("BRISK_HIP_LIB", "libbrisk_hip.so"), "mode": a.mode, "insert_ms": times, "median_ms": med(times), "entries": ck[0],
                      "sum_counts": ck[1], "digest": ck[2], "part_bits": ix.layout["part_bits"]}))
    ix.close()
    return 0


def child(job, mode, lib, steps):
    env = dict(os.environ)
    if lib:
        env["BRISK_HIP_LIB"] = lib
    else:
        env.pop("BRISK_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--one", "--mode", mode, "--steps", str(steps)] + [x for n, v in JOBS[job].items() for x in ("--" + n, str(v))]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("%s %s %s: exit %d\n%s" % (job, mode, lib, p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def high_coverage():
    """one job where the mode matters: every k-mer of a 100 kbp genome is seen ~450 (k63: ~260) times"""
    import numpy as np
    import torch

    import brisk_amd
    k, m, b, n, G = 63, 21, 14, 300_000, 100_000
    d_packed = torch.zeros((n * L + 15) // 16 + 4, dtype=torch.int32, device="cuda")
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    out = {"workload": "%d synthetic %d bp reads of a %d bp genome (%dx), k=%d m=%d b=%d" % (n, L, G, n * L // G, k, m, b)}
    for mode in ("wrap", "saturate"):
        with brisk_amd.BriskHip(k, m, b, count_mode=mode) as ix:
            ix.synth_reads(G, 0, n, L, d_packed.data_ptr(), d_starts.data_ptr())
            ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
            ix.sync()
            spec = ix.count_spectrum()
            ck = ix.checksum()
            removed = ix.prune(2, 255)
            out[mode] = {"entries": ck[0], "sum_of_stored_counts": ck[1], "spectrum_bins": {str(i): int(v) for i, v in enumerate(spec) if v},
                         "spectrum_bin_0": int(spec[0]), "spectrum_bin_1": int(spec[1]), "spectrum_bin_255": int(spec[255]),
                         "median_stored_count": int(np.searchsorted(np.cumsum(spec), (int(spec.sum()) + 1) // 2)), "prune_2_255_removed": removed}
    out["true_instances"] = n * (L - k + 1)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--mode", default="wrap", choices=("wrap", "saturate"))
    ap.add_argument("--k", type=int, default=63)
    ap.add_argument("--m", type=int, default=21)
    ap.add_argument("--b", type=int, default=14)
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="file name, inside brisk_amd/, of a build of the parent commit")
    ap.add_argument("--jobs", default=",".join(JOBS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.one:
        return one(a)
    res = {"method": "fresh processes, alternating; per process: 1 warm-up job + %d timed jobs (clear + insert_packed + sync, host clock), its median" % a.steps, "jobs": {}}
    for job in a.jobs.split(","):
        runs = {"parent": [], "default": [], "saturate": []}
        for _ in range(a.procs):
            if a.parent_lib:
                runs["parent"].append(child(job, "wrap", a.parent_lib, a.steps))
            runs["default"].append(child(job, "wrap", None, a.steps))
            runs["saturate"].append(child(job, "saturate", None, a.steps))
        j = {"config": JOBS[job]}
        for name, rs in runs.items():
            if rs:
                ms = [r["median_ms"] for r in rs]
                j[name] = {"process_medians_ms": ms, "median_ms": med(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": [r["insert_ms"] for r in rs],
                           "checksum": [rs[0]["entries"], rs[0]["sum_counts"], rs[0]["digest"]]}
        if runs["parent"]:
            spread = j["parent"]["max_ms"] - j["parent"]["min_ms"]
            j["default_vs_parent"] = {"parent_spread_ms": round(spread, 3), "delta_ms": round(j["default"]["median_ms"] - j["parent"]["median_ms"], 3),
                                      "no_slower": j["default"]["median_ms"] <= j["parent"]["median_ms"] + spread,
                                      "same_index": j["default"]["checksum"] == j["parent"]["checksum"]}
        j["saturate_vs_default"] = {"delta_ms": round(j["saturate"]["median_ms"] - j["default"]["median_ms"], 3),
                                    "ratio": round(j["saturate"]["median_ms"] / j["default"]["median_ms"], 4)}
        res["jobs"][job] = j
    res["high_coverage"] = high_coverage()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
