"""Worker of tests/test_snapshot.py, one fresh process per case (SNAPSHOT_WORKER_CASE, SNAPSHOT_WORKER_ARGS as JSON) so that a
snapshot crosses a process boundary and the library reads its environment afresh.  stdout carries `key value` lines and ends with
`ok`; a mismatch prints what differs and exits 1.

save:   count reads B of two_samples(seed) at (k, m, b, opts) and save the index to `path` (the parent loads it).
novmm:  under BRISK_NO_VMM=1 (set by the parent): save A, load it in both layouts, insert B on top; digests against the oracle's.
limit:  save A, then a handle created under BRISK_ARENA_LIMIT below A's entries: load answers ENOMEM and the handle is empty."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import brisk_amd
import oracle

ENOMEM = 4


def say(key, value):
    print(key, json.dumps(value), flush=True)


def fail(what):
    print("MISMATCH", what, flush=True)
    sys.exit(1)


def oracle_digest(O, reads, k, m, b):
    h = O.index_new(k, m, b)
    O.index_insert_reads(h, *oracle.pack_reads(reads))
    out = O.index_digest(h)
    O.index_free(h)
    return out


def main():
    from test_setops import two_samples
    case = os.environ["SNAPSHOT_WORKER_CASE"]
    args = json.loads(os.environ["SNAPSHOT_WORKER_ARGS"])
    k, m, b = args["kmb"]
    opts = args.get("opts", {})
    reads_a, reads_b = two_samples(args["seed"], **args.get("sample", {}))
    path = args["path"]
    if case == "save":
        with brisk_amd.BriskHip(k, m, b, **opts) as ix:
            ix.insert_reads(reads_b)
            say("entries", ix.save(path))
            say("checksum", ix.checksum())
    elif case == "novmm":
        assert os.environ.get("BRISK_NO_VMM") == "1"
        oracle.build(ref=False)
        O = oracle.Oracle()
        want_a, want_ab = oracle_digest(O, reads_a, k, m, b), oracle_digest(O, reads_a + reads_b, k, m, b)
        with brisk_amd.BriskHip(k, m, b, **opts) as ix:
            ix.insert_reads(reads_a)
            if ix.memory_info()["arena_reserved"] != 0:
                fail("BRISK_NO_VMM=1 but the arena has a virtual reservation")
            ix.save(path)
        for room in (False, True):
            with brisk_amd.BriskHip.open(path, room=room) as ld:
                if ld.checksum() != want_a:
                    fail(f"room={room}: loaded {ld.checksum()}, oracle {want_a}")
                ld.insert_reads(reads_b)  # the arena grows by copying what the load put there
                if ld.checksum() != want_ab:
                    fail(f"room={room}: after the insert {ld.checksum()}, oracle {want_ab}")
        say("checks", 4)
    elif case == "limit":
        with brisk_amd.BriskHip(k, m, b, **opts) as ix:
            ix.insert_reads(reads_a)
            n = ix.save(path)
        os.environ["BRISK_ARENA_LIMIT"] = str(n // 2)  # read when a handle is created
        for room in (False, True):
            with brisk_amd.BriskHip(k, m, b, **opts) as ld:
                try:
                    ld.load(path, room=room)
                    fail(f"room={room}: the load went through under BRISK_ARENA_LIMIT={n // 2}")
                except brisk_amd.BriskHipError as e:
                    if e.code != ENOMEM:
                        fail(f"room={room}: {e}")
                if ld.checksum() != (0, 0, 0) or ld.stats()["nb_kmers"] != 0 or len(ld.enumerate()[0]) != 0:
                    fail(f"room={room}: the handle is not empty after the refused load")
        say("entries", n)
    else:
        fail("unknown case " + case)
    print("ok", flush=True)


if __name__ == "__main__":
    main()
