"""Raw read intake on N reads of 150 bytes (k63 m21 b14 by default: bench.py's), for three inputs -- clean, 1 % N, 1 % N plus
qualities of which a threshold cuts about 5 % -- resident on the device:

  1. brisk_hip_intake_ascii: median wall time of the synchronous call and the kernels' own time (profile slot, HIP events on the
     handle's stream), next to two yardsticks in the same run, timed with events on the same stream: brisk_hip_pack_ascii over the
     same bases (one read of the bases, a quarter written, no cutting) and a device-to-device copy of the input bytes;
  2. from host memory, on --host-reads of the clean reads: insert_raw_reads (without and with qualities) against insert_reads;
  3. on --split-reads of the 1 % N reads: insert_raw_reads against the route a Python caller had before, a numpy split into clean
     stretches followed by insert_reads;
  4. brisk_count --bulk on a FASTQ of --fastq-reads reads, plain and gz: entries per second, the reader thread's share and rate.

Prints one JSON line (and writes it to --out).

The per-kernel split of part 1 comes from a kernel trace of `--device-only` (rocprofv3 --kernel-trace --stats), summed per kernel
and case: profiles/r20_intake_kernels.json.

    python tools/intake_bench.py [--reads 50000000] [--reps 5] [--host-reads 10000000] [--split-reads 2000000] [--fastq-reads 4000000] [--out FILE]
"""
import argparse
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import brisk_amd  # noqa: E402
from brisk_amd import hipapi  # noqa: E402

READ = 150
MIN_QUAL = 4  # qualities are uniform in 2..41: two values in forty lie below


def median(v):
    return float(np.median(v))


def make_reads(n, n_rate, dev, seed):
    """(bases, quals) uint8[n * READ] on the device, generated in pieces"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    bases = torch.empty(n * READ, dtype=torch.uint8, device=dev)
    quals = torch.empty(n * READ, dtype=torch.uint8, device=dev)
    step = 1 << 27
    for o in range(0, n * READ, step):
        m = min(step, n * READ - o)
        piece = letters[torch.randint(0, 4, (m,), device=dev, generator=g)]
        if n_rate:
            piece[torch.rand(m, device=dev, generator=g) < n_rate] = ord("N")
        bases[o:o + m] = piece
        quals[o:o + m] = (33 + torch.randint(2, 42, (m,), device=dev, generator=g)).to(torch.uint8)
    return bases, quals


def host_split(flat, n_reads, k):
    """the host route: the clean stretches of at least k bytes of reads of READ bytes, as (flat, offsets) for insert_reads"""
    valid = hipapi._IS_BASE[flat]
    at_start = np.zeros(len(flat), bool)
    at_start[::READ] = True
    begins = np.nonzero(valid & (at_start | ~np.concatenate([[False], valid[:-1]])))[0]
    ends = np.nonzero(valid & np.concatenate([at_start[1:] | ~valid[1:], [True]]))[0] + 1
    lens = ends - begins
    keep = lens >= k
    begins, lens = begins[keep], lens[keep]
    offs = np.zeros(len(lens) + 1, np.uint64)
    offs[1:] = np.cumsum(lens, dtype=np.uint64)
    src = np.repeat(begins - offs[:-1].astype(np.int64), lens) + np.arange(int(offs[-1]), dtype=np.int64)
    return np.ascontiguousarray(flat[src]), offs


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=63)
    ap.add_argument("--m", type=int, default=21)
    ap.add_argument("--b", type=int, default=14)
    ap.add_argument("--host-reads", type=int, default=10_000_000)
    ap.add_argument("--split-reads", type=int, default=2_000_000)
    ap.add_argument("--fastq-reads", type=int, default=4_000_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true", help="part 1 only: what a kernel trace of the intake is taken over")
    a = ap.parse_args()
    n, nb = a.reads, a.reads * READ
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ix = brisk_amd.BriskHip(a.k, a.m, a.b, stream=stream.cuda_stream)
    L = ix.L
    res = {"reads": n, "bytes": nb, "k": a.k, "m": a.m, "b": a.b, "reps": a.reps, "min_qual": MIN_QUAL, "intake_block": brisk_amd.INTAKE_BLOCK}

    d_offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * READ
    cap_words, frag_cap = (nb + 15) // 16 + 2, nb // a.k
    d_packed = torch.empty(cap_words + 2, dtype=torch.int32, device=dev)
    d_starts = torch.empty(frag_cap + 1, dtype=torch.int64, device=dev)
    d_frags = torch.empty(2 * frag_cap, dtype=torch.int64, device=dev)
    d_copy = torch.empty(nb, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def events(fn):
        t = []
        for rep in range(a.reps + 1):  # the first is a warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        return median(t[1:])

    host = {}
    for name, n_rate, with_q in (("clean", 0.0, False), ("n1", 0.01, False), ("n1_q5", 0.01, True)):
        bases, quals = make_reads(n, n_rate, dev, 1 if n_rate == 0 else 2)
        torch.cuda.synchronize()
        rule = brisk_amd.intake_rule(min_qual=MIN_QUAL if with_q else 0)
        wall, kern = [], []
        for rep in range(a.reps + 1):
            ix.profile_reset()
            ix.profile_enable(True)
            t0 = time.perf_counter()
            st = ix.intake_ascii(bases.data_ptr(), quals.data_ptr() if with_q else 0, d_offsets.data_ptr(), n, rule, d_packed.data_ptr(), cap_words, d_starts.data_ptr(),
                                 d_frags.data_ptr(), frag_cap)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(ix.profile_read()["k_intake_mask_count_apply_gather"]["ms"])
            ix.profile_enable(False)
        assert st["n_bases_in"] == nb == st["n_nts"] + st["n_cut_base"] + st["n_cut_qual"] + st["n_short"]
        pack_ms = events(lambda: ix.pack_ascii(bases.data_ptr(), nb, d_packed.data_ptr()))
        with torch.cuda.stream(stream):
            copy_ms = events(lambda: d_copy.copy_(bases))
        # the byte model: bases once in the mask pass and the kept ones once in the gather; qualities once; the mask
        # word (4 bytes per 16) zeroed, read and written by the mask pass, read by the count and the apply pass (five times in all: a
        # lane's look at its successor's word hits the line it shares with it); the packed output; 80 bytes per fragment of table
        in_bytes = nb * (1 + st["n_nts"] / nb + (1 if with_q else 0)) + nb / 4 * 5 + st["n_nts"] / 4 + st["n_fragments"] * 80
        row = {"stats": st, "wall_ms": median(wall[1:]), "kernels_ms": median(kern[1:]), "pack_ascii_ms": pack_ms, "dtod_copy_ms": copy_ms, "model_bytes": in_bytes,
               "model_GBps_wall": in_bytes / median(wall[1:]) / 1e6, "model_GBps_kernels": in_bytes / median(kern[1:]) / 1e6, "pack_ascii_GBps": nb * 1.25 / pack_ms / 1e6,
               "dtod_copy_GBps": 2 * nb / copy_ms / 1e6, "ratio_to_pack_ascii_wall": median(wall[1:]) / pack_ms, "ratio_to_pack_ascii_kernels": median(kern[1:]) / pack_ms}
        res["intake_ascii_" + name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)
        keep = 0 if a.device_only else max(a.host_reads, a.split_reads, a.fastq_reads) * READ
        host[name] = (bases[:keep].cpu().numpy(), quals[:keep].cpu().numpy())
        del bases, quals
    del d_packed, d_starts, d_frags, d_copy, d_offsets
    torch.cuda.empty_cache()
    ix.close()
    if a.device_only:
        print(json.dumps(res))
        return 0

    def timed_insert(fn):
        t = []
        for rep in range(6):  # the first is a warm-up (buffers grow)
            with brisk_amd.BriskHip(a.k, a.m, a.b) as h:
                t0 = time.perf_counter()
                fn(h)
                h.sync()
                t.append(time.perf_counter() - t0)
                entries = h.stats()["nb_kmers"]
        return median(t[1:]), entries

    def raw(h, flat, qflat, offs, min_qual=0):
        st = hipapi._IntakeStats()
        rule = brisk_amd.intake_rule(min_qual=min_qual)
        h._chk(L.brisk_hip_insert_raw_reads(h.h, C.c_void_p(flat.ctypes.data), None if qflat is None else C.c_void_p(qflat.ctypes.data), offs, len(offs) - 1, C.byref(rule), C.byref(st)))

    # 2. clean reads from host memory
    hn = min(a.host_reads, n)
    flat, qflat = host["clean"][0][:hn * READ], host["clean"][1][:hn * READ]
    offs = np.arange(hn + 1, dtype=np.uint64) * np.uint64(READ)
    t_reads, e0 = timed_insert(lambda h: h.insert_flat(flat, offs))
    t_raw, e1 = timed_insert(lambda h: raw(h, flat, None, offs))
    t_rawq, e2 = timed_insert(lambda h: raw(h, flat, qflat, offs, 1))  # (every quality is >= 35: nothing is cut, the bytes travel)
    assert e0 == e1 == e2
    res["host_clean"] = {"reads": hn, "entries": e0, "insert_reads_s": t_reads, "insert_raw_s": t_raw, "insert_raw_with_quals_s": t_rawq, "raw_over_reads": t_raw / t_reads,
                         "raw_with_quals_over_reads": t_rawq / t_reads}
    # 3. 1 % N: the device cut against a host split
    sn = min(a.split_reads, n)
    flat = host["n1"][0][:sn * READ]
    offs = np.arange(sn + 1, dtype=np.uint64) * np.uint64(READ)
    t0 = time.perf_counter()
    sflat, soffs = host_split(flat, sn, a.k)
    t_split = time.perf_counter() - t0
    t_ins, e0 = timed_insert(lambda h: h.insert_flat(sflat, soffs))
    t_raw, e1 = timed_insert(lambda h: raw(h, flat, None, offs))
    assert e0 == e1
    res["host_n1"] = {"reads": sn, "entries": e0, "numpy_split_s": t_split, "insert_reads_of_the_split_s": t_ins, "host_route_s": t_split + t_ins, "insert_raw_s": t_raw,
                      "host_route_over_raw": (t_split + t_ins) / t_raw}
    # 4. brisk_count --bulk on a FASTQ
    fq = min(a.fastq_reads, n)
    exe = brisk_amd.build_apps()["brisk_count"] if not os.path.exists(os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")) else os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    with tempfile.TemporaryDirectory() as tmp:
        rec = np.empty((fq, 3 + READ + 3 + READ + 1), np.uint8)
        rec[:, :3] = np.frombuffer(b"@r\n", np.uint8)
        rec[:, 3:3 + READ] = host["n1_q5"][0][:fq * READ].reshape(fq, READ)
        rec[:, 3 + READ:6 + READ] = np.frombuffer(b"\n+\n", np.uint8)
        rec[:, 6 + READ:6 + 2 * READ] = host["n1_q5"][1][:fq * READ].reshape(fq, READ)
        rec[:, -1] = ord("\n")
        plain = os.path.join(tmp, "reads.fq")
        rec.tofile(plain)
        gz = plain + ".gz"
        with gzip.open(gz, "wb", compresslevel=1) as f:
            f.write(rec.tobytes())
        for name, path in (("plain", plain), ("gz", gz)):
            p = subprocess.run([exe, "--bulk", path, str(a.k), str(a.m), str(a.b), "-", "--min-qual", str(MIN_QUAL)], capture_output=True, text=True, env=dict(os.environ, BRISK_E2E_JSON="1"))
            assert p.returncode == 0, p.stderr
            e2e = json.loads([l for l in p.stdout.splitlines() if l.startswith("E2E ")][0][4:])
            res["brisk_count_fastq_" + name] = dict(e2e, reads=fq, file_bytes=os.path.getsize(path), entries_per_s=e2e["entries"] / e2e["wall_s"],
                                                    reader_share=e2e["reader_produce_s"] / e2e["wall_s"], reader_MBps_inflated=rec.nbytes / e2e["reader_produce_s"] / 1e6)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
