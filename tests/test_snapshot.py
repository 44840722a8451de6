"""GPU: index snapshots (save, load in both layouts, open) against the CPU oracle, bit-exact.

Expected values never come from the library under test: they are the oracle's index_dump of the reads (tests/test_setops.py's
two_samples and joins), Oracle.digest_entries for checksums, want_stats for nb_kmers / nb_buckets, expected_all for per-k-mer
answers.  Saved files are parsed by tests/snapshot_reader.py, a reader written from DESIGN.md section 4.w.  Where a test compares
the library with itself (enumeration order across a round trip, byte-identical files) it says so.

Geometries: the six of tests/test_spectrum_prune.py plus k47 m13 b8 with part_bits = 4 (thousands of entries in each of 16
partitions: a partition spans several tiles of k_snapshot_move)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle
import snapshot_reader
from test_setops import ALL_GEOMS, ALL_IDS, as_dict, as_dump, expected, expected_compare, inputs, two_samples
from test_spectrum_prune import keep, oracle_index, partition_of, same_multiset, want_stats

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, EIO, EFORMAT = 1, 4, 7, 8
TESTS = os.path.dirname(os.path.abspath(__file__))
PB4 = ALL_GEOMS[6]


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


def same_sequence(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def check_is(O, ix, ha, want):
    """the index holds exactly the entries `want` (an oracle dump)"""
    assert ix.checksum() == O.digest_entries(*want)
    st = ix.stats()
    assert (st["nb_kmers"], st["nb_buckets"]) == want_stats(O, ha, want)
    assert same_multiset(ix.enumerate(), want)
    assert np.array_equal(ix.count_spectrum(), np.bincount(want[3], minlength=256).astype(np.uint64))


def code_of(call):
    import brisk_amd
    with pytest.raises(brisk_amd.BriskHipError) as e:
        call()
    return e.value.code, str(e.value)


# ---- 1: round trip -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts", ALL_GEOMS, ids=ALL_IDS)
def test_round_trip(B, O, tmp_path, kmb, opts):
    from test_kmer_query import as_u16, assert_slots, expected_all
    k, m, b = kmb
    reads_a, reads_b, ha, da, db = inputs(O, kmb, opts)
    want = O.index_dump(ha)
    path = tmp_path / "a.snap"
    with B.BriskHip(k, m, b, **opts) as ix:
        ix.insert_reads(reads_a)
        saved = ix.enumerate()
        skm, lay = ix.stats()["nb_skmers"], ix.layout
        assert ix.save(path) == len(want[0])
    info = B.snapshot_info(path)
    assert info["n_entries"] == len(want[0]) and info["checksum"] == O.digest_entries(*want) and info["nb_skmers"] == skm
    queries = [q.upper() for q in reads_a[:70] + reads_b[:50]]
    qf, qo = oracle.pack_reads(queries)
    slots, alts, base = expected_all(O, ha, queries, k, m)
    rng = np.random.default_rng(k)
    pick = rng.choice(len(want[0]), 300, replace=False)
    for room in (False, True):
        with B.BriskHip.open(path, room=room) as ld:
            assert ld.layout == lay, room
            check_is(O, ld, ha, want)
            assert same_sequence(ld.enumerate(), saved), room  # the library against itself: enumeration order is kept
            assert ld.stats()["nb_skmers"] == skm
            assert np.array_equal(ld.get_reads(queries), O.index_query_reads(ha, qf, qo)), room
            counts, found, got_base = ld.get_kmers(queries)
            assert np.array_equal(got_base, base)
            assert_slots(as_u16(counts, found), slots, alts, (kmb, room))
            data, fnd = ld.lookup(want[0][pick], want[1][pick], want[2][pick])
            assert fnd.all() and np.array_equal(data, want[3][pick]), room
            absent = [x for x in db if x not in da][:100]
            lo, hi, idx = (np.array(v, dt) for v, dt in zip(zip(*[(x[1], x[0], x[2]) for x in absent]), (np.uint64, np.uint64, np.uint8)))
            assert not ld.lookup(lo, hi, idx)[1].any(), room
    O.index_free(ha)


# ---- 2: the index afterwards -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts", ALL_GEOMS, ids=ALL_IDS)
def test_insert_after_load(B, O, tmp_path, kmb, opts):
    k, m, b = kmb
    reads_a, reads_b, ha, da, db = inputs(O, kmb, opts, seed_shift=1)
    hab = oracle_index(O, reads_a + reads_b, k, m, b)  # the oracle index that received A, then B
    want = O.index_dump(hab)
    path = tmp_path / "a.snap"
    with B.BriskHip(k, m, b, **opts) as ix:
        ix.insert_reads(reads_a)
        ix.save(path)
    for room in (False, True):
        with B.BriskHip.open(path, room=room) as ld:
            ld.insert_reads(reads_b)
            check_is(O, ld, hab, want)
            left = keep(want, 2, 255)
            assert ld.prune(2, 255) == len(want[0]) - len(left[0])
            check_is(O, ld, hab, left)
    O.index_free(ha)
    O.index_free(hab)


@pytest.mark.parametrize("kmb,opts", [ALL_GEOMS[0], ALL_GEOMS[1], ALL_GEOMS[2], PB4], ids=[ALL_IDS[0], ALL_IDS[1], ALL_IDS[2], ALL_IDS[6]])
def test_saving_an_index_with_holes(B, O, tmp_path, kmb, opts):
    k, m, b = kmb
    reads_a, reads_b, ha, da, db = inputs(O, kmb, opts, seed_shift=2)
    left = as_dump({x: c for x, c in da.items() if c >= 2 and x not in db})
    assert 0 < len(left[0]) < len(da) * 3 // 4
    path = tmp_path / "holes.snap"
    with B.BriskHip(k, m, b, **opts) as ix, B.BriskHip(k, m, b, **opts) as sub:
        ix.insert_reads(reads_a)
        sub.insert_reads(reads_b)
        ix.prune(2, 255)
        ix.subtract(sub)
        order = ix.enumerate()
        assert ix.save(path) == len(left[0])
    assert B.snapshot_info(path)["n_entries"] == len(left[0])  # the survivors only
    hdr, blocks = snapshot_reader.read(path)
    assert sum(len(bk["data"]) for bk in blocks) == len(left[0])
    for room in (False, True):
        with B.BriskHip.open(path, room=room) as ld:
            check_is(O, ld, ha, left)
            assert same_sequence(ld.enumerate(), order)  # the library against itself
    O.index_free(ha)


# ---- 3: set operations with a source that another process saved -------------------------------------------------------------------------
def _worker(case, args, extra_env=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if not k.startswith("BRISK_") or k == "BRISK_HIP_LIB"}
    env.update(extra_env or {}, SNAPSHOT_WORKER_CASE=case, SNAPSHOT_WORKER_ARGS=json.dumps(args))
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(TESTS, "snapshot_worker.py")], env=env, capture_output=True, text=True, timeout=timeout)
    print(f"snapshot_worker {case}: {time.time() - t0:.0f} s")
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout[-6000:], p.stderr[-6000:])


@pytest.mark.parametrize("kmb,opts", [ALL_GEOMS[0], ALL_GEOMS[2]], ids=[ALL_IDS[0], ALL_IDS[2]])
def test_set_operations_from_a_loaded_index(B, O, tmp_path, kmb, opts):
    k, m, b = kmb
    seed = k * 100 + m + 3
    reads_a, reads_b, ha, da, db = inputs(O, kmb, opts, seed_shift=3)
    path = str(tmp_path / "b.snap")
    _worker("save", dict(kmb=kmb, opts=opts, seed=seed, path=path))  # B counted and saved by a child process
    assert B.snapshot_info(path)["checksum"] == O.digest_entries(*as_dump(db))
    for op, rule in (("merge", "left"), ("intersect", "min"), ("compare", "left")):
        with B.BriskHip(k, m, b, **opts) as ix, B.BriskHip.open(path) as src:
            ix.insert_reads(reads_a)
            if op == "compare":
                assert ix.compare(src) == expected_compare(da, db)
                continue
            got_n = ix.merge(src) if op == "merge" else ix.intersect(src, count=rule)
            want = as_dump(expected(op, da, db, rule))
            assert got_n == abs(len(want[0]) - len(da))
            check_is(O, ix, ha, want)
            assert src.checksum() == O.digest_entries(*as_dump(db))
    O.index_free(ha)


# ---- 4: what save does to its index, and deferred inserts ---------------------------------------------------------------------------------
def test_source_untouched_and_two_saves_are_the_same_bytes(B, O, tmp_path):
    k, m, b = 63, 21, 14
    reads_a, _ = two_samples(11)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(reads_a)
        ix.prune(1, 200)
        # (memory_bytes is left out: it counts the handle's scratch buffers, which a save, like an enumerate, may grow)
        index_stats = lambda: {name: v for name, v in ix.stats().items() if name != "memory_bytes"}
        cs, order, st = ix.checksum(), ix.enumerate(), index_stats()
        ix.save(tmp_path / "one.snap")
        assert ix.checksum() == cs and same_sequence(ix.enumerate(), order) and index_stats() == st
        ix.save(tmp_path / "two.snap")
        assert ix.checksum() == cs and same_sequence(ix.enumerate(), order)
    assert (tmp_path / "one.snap").read_bytes() == (tmp_path / "two.snap").read_bytes()
    assert sorted(os.listdir(tmp_path)) == ["one.snap", "two.snap"]  # no temporary file stays behind


def test_deferred_inserts_are_in_the_file(B, O, tmp_path):
    k, m, b = 63, 21, 14
    reads_a, _ = two_samples(12)
    ha = oracle_index(O, reads_a, k, m, b)
    want = O.index_dump(ha)
    with B.BriskHip(k, m, b) as ix:  # default options: these small batches are deferred
        for i in range(0, len(reads_a), 200):
            ix.insert_reads(reads_a[i:i + 200])
        assert ix.save(tmp_path / "d.snap") == len(want[0])  # no call in between
    info = B.snapshot_info(tmp_path / "d.snap")
    assert info["n_entries"] == len(want[0]) and info["checksum"] == O.digest_entries(*want)
    with B.BriskHip.open(tmp_path / "d.snap") as ld:
        check_is(O, ld, ha, want)
    O.index_free(ha)


# ---- 5: blocks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts,limit", [PB4 + (1000,), ALL_GEOMS[0] + (64,)], ids=[ALL_IDS[6] + "-1000", ALL_IDS[0] + "-64"])
def test_blocks(B, O, tmp_path, monkeypatch, kmb, opts, limit):
    k, m, b = kmb
    reads_a, reads_b, ha, da, db = inputs(O, kmb, opts, seed_shift=4)
    want = O.index_dump(ha)
    with B.BriskHip(k, m, b, **opts) as ix:
        ix.insert_reads(reads_a)
        order = ix.enumerate()
        monkeypatch.delenv("BRISK_SNAPSHOT_BLOCK", raising=False)
        ix.save(tmp_path / "default.snap")
        monkeypatch.setenv("BRISK_SNAPSHOT_BLOCK", str(limit))  # read at each save
        ix.save(tmp_path / "small.snap")
    monkeypatch.delenv("BRISK_SNAPSHOT_BLOCK")
    h0, b0 = snapshot_reader.read(tmp_path / "default.snap")
    h1, b1 = snapshot_reader.read(tmp_path / "small.snap")
    assert len(b0) == 1 and len(b1) > 10 and h1["n_blocks"] == len(b1)
    assert {x: v for x, v in h0.items() if x != "n_blocks"} == {x: v for x, v in h1.items() if x != "n_blocks"}  # same n_entries, same digest
    cat = lambda bs, name: np.concatenate([bk[name] for bk in bs])
    assert all(np.array_equal(cat(b0, name), cat(b1, name)) for name in ("partitions", "counts", "keys", "data"))  # only the block structure differs
    sizes = [len(bk["data"]) for bk in b1]
    assert all(n <= limit or len(bk["counts"]) == 1 for n, bk in zip(sizes, b1))  # within the limit, or one partition on its own
    firsts = [int(bk["partitions"][0]) for bk in b1]
    assert firsts == sorted(firsts) and all(int(x["partitions"][-1]) < int(y["partitions"][0]) for x, y in zip(b1, b1[1:]))
    if opts.get("part_bits") == 4:
        assert max(sizes) > limit  # a partition larger than the limit is a block of its own
    for room in (False, True):
        with B.BriskHip.open(tmp_path / "small.snap", room=room) as ld:
            check_is(O, ld, ha, want)
            assert same_sequence(ld.enumerate(), order)  # the library against itself
    O.index_free(ha)


# ---- 6: the format, read independently ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts", ALL_GEOMS, ids=ALL_IDS)
def test_format_read_by_an_independent_reader(B, O, tmp_path, kmb, opts):
    k, m, b = kmb
    reads_a, reads_b, ha, da, db = inputs(O, kmb, opts, seed_shift=5)
    want = O.index_dump(ha)
    path = tmp_path / "f.snap"
    with B.BriskHip(k, m, b, **opts) as ix:
        ix.insert_reads(reads_a)
        lay = ix.layout
        ix.save(path)
    hdr, blocks = snapshot_reader.read(path)
    for name in ("k", "m", "b", "part_bits", "ext_bits", "cls_bits", "cls_width"):
        assert hdr[name] == lay[name], name
    assert hdr["data_bytes"] == 1 and hdr["shift"] == 2 * b + lay["ext_bits"] - lay["part_bits"]
    assert hdr["key_words"] == (1 if hdr["shift"] + 2 * (k - b) + 6 <= 64 else 2)
    assert hdr["checksum"] == O.digest_entries(*want)
    parts = np.concatenate([bk["partitions"] for bk in blocks]).astype(np.int64)
    counts = np.concatenate([bk["counts"] for bk in blocks]).astype(np.int64)
    assert (np.diff(parts) > 0).all() and parts.max() < (1 << hdr["part_bits"]) and counts.min() >= 1
    assert counts.sum() == hdr["n_entries"] == len(want[0]) and len(parts) == hdr["n_partitions"]
    assert all(bk["counts"].sum() == len(bk["data"]) == len(bk["keys"]) for bk in blocks)
    if lay["ext_bits"] == lay["cls_bits"]:  # per-partition counts from the oracle's bucket ids
        p_want, c_want = np.unique(partition_of(O, ha, want, lay), return_counts=True)
        assert np.array_equal(parts, p_want) and np.array_equal(counts, c_want)
    data = np.concatenate([bk["data"] for bk in blocks])
    assert np.array_equal(np.bincount(data, minlength=256), np.bincount(want[3], minlength=256))
    size = snapshot_reader.HEADER_BYTES + sum(snapshot_reader.block_bytes(len(bk["counts"]), len(bk["data"]), hdr["key_words"]) for bk in blocks)
    assert os.path.getsize(path) == size
    if not opts:  # sparse on purpose: a few thousand entries in 2^24 partitions are not a 64 MB file
        assert size < 40 * len(want[0]) + 4096
    O.index_free(ha)


def test_empty_index(B, tmp_path):
    with B.BriskHip(31, 15, 14) as ix:
        assert ix.save(tmp_path / "e.snap") == 0
    assert os.path.getsize(tmp_path / "e.snap") == snapshot_reader.HEADER_BYTES
    for room in (False, True):
        with B.BriskHip.open(tmp_path / "e.snap", room=room) as ld:
            assert ld.checksum() == (0, 0, 0) and ld.stats()["nb_kmers"] == 0 and len(ld.enumerate()[0]) == 0
            ld.insert_reads(["ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGGCTAGCTAGCTAGG"])
            assert ld.checksum()[0] > 0


# ---- 7: refusals, each leaving the target empty and usable -----------------------------------------------------------------------------------
def test_refusals(B, O, tmp_path):
    k, m, b, opts = 31, 15, 8, dict(part_bits=12)
    reads_a, _ = two_samples(13)
    ha = oracle_index(O, reads_a, k, m, b)
    want = O.index_dump(ha)
    good = tmp_path / "good.snap"
    with B.BriskHip(k, m, b, **opts) as ix:
        ix.insert_reads(reads_a)
        ix.save(good)
        cs = ix.checksum()
        code, msg = code_of(lambda: ix.load(good))  # not empty
        assert code == EINVAL and "load into an empty index, or load into a second handle and merge" in msg and ix.checksum() == cs
        code, msg = code_of(lambda: ix.save(tmp_path / "no_such_dir" / "x.snap"))
        assert code == EIO and ix.checksum() == cs
    assert sorted(os.listdir(tmp_path)) == ["good.snap"]  # no file appears
    raw = good.read_bytes()
    hdr, blocks = snapshot_reader.read(good)
    bk = blocks[0]
    keys_at = bk["offset"] + 16 + 8 * len(bk["counts"])
    data_at = keys_at + 8 * hdr["key_words"] * len(bk["data"])

    def flipped(at):
        x = bytearray(raw)
        x[at] ^= 0x10
        return bytes(x)
    bad = {"truncated": (raw[:data_at - 40], EIO, ""), "magic": (b"BRISKSNP" + raw[8:], EFORMAT, ""), "count": (flipped(data_at + 5), EFORMAT, "digest"),
           "key": (flipped(keys_at + 8 * 7 + 1), EFORMAT, "digest")}
    with B.BriskHip(k, m, b, **opts) as ld:
        for name, (content, want_code, word) in bad.items():
            (tmp_path / (name + ".snap")).write_bytes(content)
            code, msg = code_of(lambda: ld.load(tmp_path / (name + ".snap")))
            assert code == want_code and word in msg, (name, code, msg)
            assert ld.checksum() == (0, 0, 0) and ld.stats()["nb_kmers"] == 0, name  # the empty index ...
            assert ld.load(good) == len(want[0]) and ld.checksum() == cs, name  # ... and usable
            ld.clear()
    for other, word in ((dict(k=31, m=13, b=8, part_bits=12), " m"), (dict(k=31, m=15, b=8, part_bits=13), "part_bits")):
        with B.BriskHip(**other) as ld:
            code, msg = code_of(lambda: ld.load(good))
            assert code == EINVAL and word in msg, (other, msg)
            assert ld.checksum() == (0, 0, 0)
            ld.insert_reads(reads_a[:20])  # usable
            assert ld.checksum()[0] > 0
    with B.BriskHip(k, m, b, entry_ids=True, **opts) as ld:
        for call in (lambda: ld.load(good), lambda: ld.save(tmp_path / "ids.snap")):
            code, msg = code_of(call)
            assert code == EINVAL and "entry-id" in msg
    with B.BriskHip(k, m, b, n_owners=2, **opts) as ld:
        assert code_of(lambda: ld.load(good))[0] == EINVAL and code_of(lambda: ld.save(tmp_path / "sh.snap"))[0] == EINVAL
    assert not (tmp_path / "ids.snap").exists() and not (tmp_path / "sh.snap").exists()
    O.index_free(ha)


# ---- 8: arena paths (a child process each: the library reads these settings when a handle is created) -------------------------------------------
def test_copy_growth_arena(tmp_path):
    _worker("novmm", dict(kmb=(63, 21, 14), seed=21, path=str(tmp_path / "a.snap")), {"BRISK_NO_VMM": "1"})


def test_arena_limit(tmp_path):
    _worker("limit", dict(kmb=(31, 15, 14), seed=22, path=str(tmp_path / "a.snap")))


# ---- 9: the app -------------------------------------------------------------------------------------------------------------------------------
def test_app_save_load_and_set_operations(B, O, tmp_path):
    exe = os.path.join(os.path.dirname(TESTS), "brisk_amd", "apps", "brisk_count")
    apps = {"brisk_count": exe} if os.path.exists(exe) else B.build_apps()
    k, m, b = 31, 15, 14
    reads_a, reads_b, ha, da, db = inputs(O, (k, m, b), {}, seed_shift=6)
    for name, reads in (("A", reads_a), ("B", reads_b)):
        (tmp_path / (name + ".fa")).write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(reads) if r))
    env = {x: v for x, v in os.environ.items() if not x.startswith("BRISK_") or x == "BRISK_HIP_LIB"}
    t = lambda name: str(tmp_path / name)

    def run(*args):
        return subprocess.run([apps["brisk_count"], "--bulk"] + list(args), env=env, capture_output=True, text=True, timeout=300)
    kmb = [str(k), str(m), str(b)]
    for name in ("A", "B"):
        p = run(t(name + ".fa"), *kmb, t("dump" + name), "--save", t(name + ".snap"))
        assert p.returncode == 0, (p.stdout, p.stderr)
    assert open(t("dumpA")).read().split("\n")[:-1] == oracle.multiset_lines(*as_dump(da), k)
    assert B.snapshot_info(t("B.snap"))["checksum"] == O.digest_entries(*as_dump(db))
    p = run("-", *kmb, t("dump2"), "--load", t("A.snap"), "--merge", t("B.snap"))
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert open(t("dump2")).read().split("\n")[:-1] == oracle.multiset_lines(*as_dump(expected("merge", da, db)), k)
    p = run("-", *kmb, t("dump3"), "--load", t("A.snap"), "--subtract", t("A.snap"))
    assert p.returncode == 0 and open(t("dump3")).read() == "" and "nb_kmers 0 " in p.stdout, (p.stdout, p.stderr)
    p = run(t("B.fa"), *kmb, t("dump4"), "--load", t("A.snap"))  # reads counted on top of a snapshot
    assert p.returncode == 0 and open(t("dump4")).read().split("\n")[:-1] == oracle.multiset_lines(*as_dump(expected("merge", da, db)), k), (p.stdout, p.stderr)
    p = run("-", "31", "15", "12", "-", "--load", t("A.snap"))
    assert p.returncode == 2, (p.returncode, p.stdout, p.stderr)
    O.index_free(ha)
