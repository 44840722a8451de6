"""Index snapshots: whole save and whole load (both layouts) of a synthetic index, against yardsticks that do not run the code
under test, in one process.

    python tools/snapshot_bench.py [--reads 20000000 --k 63 --m 21 --b 14] [--coverage 15] [--reps 3] [--dir /dev/shm] [--out FILE]

The index is bench.py's kind: synthetic 150-nt reads of one genome, inserted from device memory.  Every measured call is
synchronous (save and load return when the file, or the index, is whole), so the host clock around it is the whole call.
  save_ms / load_compact_ms / load_room_ms   brisk_hip_save / brisk_hip_load, every value of --reps rounds and the median
  d2d_copy_ms     torch copy of as many bytes as the index's entries, device to device (what a gather could at best approach)
  d2h_copy_ms / h2d_copy_ms   the same bytes over PCIe through pinned memory, one copy (the floor of a save / load without a file)
  file_write_ms / file_read_ms   the same bytes from host memory to the file and back (the file system's share), with its path and kind
  recount_ms      insert_packed of the reads again: what a user does without a snapshot
Not measured here (named as missing in the output): k_snapshot_move alone -- it has no entry point of its own; a
`rocprofv3 --kernel-trace --stats` run of this tool gives its time per block.
Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import brisk_amd  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stat(v):
    return {"median": round(sorted(v)[len(v) // 2], 3), "min": round(min(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def fs_kind(path):
    best = ("", "unknown")
    for line in open("/proc/mounts"):
        f = line.split()
        if os.path.abspath(path).startswith(f[1]) and len(f[1]) > len(best[0]):
            best = (f[1], f[2])
    return best[1]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=63)
    ap.add_argument("--m", type=int, default=21)
    ap.add_argument("--b", type=int, default=14)
    ap.add_argument("--part-bits", type=int, default=0)
    ap.add_argument("--coverage", type=float, default=15.0)
    ap.add_argument("--prune", type=int, default=0, help="prune(N, 255) before saving")
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, L = a.reads, 150
    G = max(int(n * L / a.coverage), L + 1)
    path = os.path.join(a.dir, "brisk_snapshot_bench.%d.snap" % os.getpid())
    res = {"workload": "%d synthetic %d bp reads of a genome of %d nt, k=%d m=%d b=%d part_bits=%d prune=%d" % (n, L, G, a.k, a.m, a.b, a.part_bits, a.prune),
           "file": {"dir": a.dir, "kind": fs_kind(a.dir)}, "missing": ["k_snapshot_move alone (no entry point of its own: rocprofv3 --kernel-trace --stats of this tool)"]}
    ix = brisk_amd.BriskHip(a.k, a.m, a.b, part_bits=a.part_bits, immediate_inserts=True)
    d_packed = torch.zeros((n * L + 15) // 16 + 4, dtype=torch.int32, device="cuda")
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.synth_reads(G, 0, n, L, d_packed.data_ptr(), d_starts.data_ptr())
    ix.sync()

    def count():
        ix.clear()
        ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
        ix.sync()
    count()  # warm-up
    res["recount_ms"] = stat([timed(count)[0] for _ in range(a.reps)])
    if a.prune:
        res["pruned"] = ix.prune(a.prune, 255)
    cs = ix.checksum()
    ix.save(path)  # warm-up
    info = brisk_amd.snapshot_info(path)
    nbytes = info["n_entries"] * (8 * info["key_words"] + 1)
    res.update(entries=info["n_entries"], partitions=info["n_partitions"], blocks=info["n_blocks"], file_bytes=info["file_bytes"], entry_bytes=nbytes)
    res["save_ms"] = stat([timed(lambda: ix.save(path))[0] for _ in range(a.reps)])
    for name, room in (("load_compact_ms", False), ("load_room_ms", True)):
        v = []
        with brisk_amd.BriskHip(a.k, a.m, a.b, part_bits=a.part_bits, immediate_inserts=True) as ld:
            ld.load(path, room=room)  # warm-up: the arena is mapped once, as for an index that is reused
            assert ld.checksum() == cs
            for _ in range(a.reps):
                ld.clear()
                v.append(timed(lambda: ld.load(path, room=room))[0])
            res[name.replace("_ms", "_arena_mapped")] = ld.memory_info()["arena_mapped"]
        res[name] = stat(v)
    # yardsticks over the same number of bytes; none of them runs the library
    chunk = min(nbytes, 1 << 30)
    src = torch.empty(chunk, dtype=torch.uint8, device="cuda")
    dst = torch.empty(chunk, dtype=torch.uint8, device="cuda")
    pin = torch.empty(chunk, dtype=torch.uint8).pin_memory()
    scale = nbytes / chunk
    dst.copy_(src)
    res["d2d_copy_ms"] = stat([timed(lambda: dst.copy_(src))[0] * scale for _ in range(a.reps)])
    res["d2h_copy_ms"] = stat([timed(lambda: pin.copy_(src, non_blocking=True))[0] * scale for _ in range(a.reps)])
    res["h2d_copy_ms"] = stat([timed(lambda: dst.copy_(pin, non_blocking=True))[0] * scale for _ in range(a.reps)])
    raw = open(path, "rb").read(chunk)
    tmp = path + ".raw"

    def write():
        with open(tmp, "wb") as f:
            f.write(raw)
    res["file_write_ms"] = stat([timed(write)[0] * scale for _ in range(a.reps)])
    res["file_read_ms"] = stat([timed(lambda: open(tmp, "rb").read())[0] * scale for _ in range(a.reps)])
    res["yardstick_bytes"] = {"measured": chunk, "scaled_to": nbytes}
    os.unlink(tmp)
    os.unlink(path)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
