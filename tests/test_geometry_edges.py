"""GPU: everything that decodes an entry's key, at the geometries where the key layout, the record and the scan change their code
path (tests/geometry_edges.py: keys of exactly 64, of 66 and of 128 bits, a routing field across the word boundary, records of 1 and
of 4 words, k = 32 and 33, minimizer_idx classes).  Expected values never come from the library under test: they are the oracle's
dump, digest, per-read sums and per-slot answers of the same reads, joined and filtered in Python by the helpers of
test_setops.py, test_spectrum_prune.py and test_kmer_query.py; saved files are parsed by tests/snapshot_reader.py.  Every test
first asserts that the library lays the row out as the formula says (BriskHip.layout, snapshot_info of a file it saved)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import geometry_edges as G
import snapshot_reader
from test_kmer_query import as_u16, assert_slots, expected_all
from test_setops import as_dump, expected, expected_compare
from test_spectrum_prune import keep, oracle_index, same_multiset, want_stats

pytestmark = pytest.mark.gpu

EINVAL = 1
TESTS = os.path.dirname(os.path.abspath(__file__))
ROWS = pytest.mark.parametrize("r", G.TABLE, ids=[G.row_id(r) for r in G.TABLE])
ORDER_FREE = ("n_kmers", "n_present", "n_solid", "min_present", "max_present", "median", "median_present", "sum")


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


def filled(B, r, tmp_path, reads, **kw):
    """an index of `reads`, inserted in two batches, whose layout is the formula's: ix.layout, and the header of a file it saved"""
    ix = B.BriskHip(r.k, r.m, r.b, **G.opts(r), **kw)
    half = len(reads) // 2
    ix.insert_reads(reads[:half])
    ix.insert_reads(reads[half:])  # the second batch meets existing entries
    path = tmp_path / "layout.snap"
    ix.save(path)
    G.check_library_layout(r, ix.layout, B.snapshot_info(path))
    return ix


def check_is(O, ix, h, want):
    """the index holds exactly the entries `want` (a dump): multiset, checksum, nb_kmers / nb_buckets, spectrum"""
    assert same_multiset(ix.enumerate(), want)
    assert ix.checksum() == O.digest_entries(*want)
    st = ix.stats()
    assert (st["nb_kmers"], st["nb_buckets"]) == want_stats(O, h, want)
    assert np.array_equal(ix.count_spectrum(), np.bincount(want[3], minlength=256).astype(np.uint64))


def check_get_kmers(ix, c, slots=None, alts=None, what=""):
    counts, found, base = ix.get_kmers(c.queries)
    assert np.array_equal(base, c.base)
    assert_slots(as_u16(counts, found), c.slots if slots is None else slots, c.alts if alts is None else alts, what)


# ---- index ---------------------------------------------------------------------------------------------------------------------
def index_family(B, O, tmp_path, r):
    c = G.case(O, r)
    lo, hi, idx, cnt = c.dump_a
    with filled(B, r, tmp_path, c.reads_a) as ix:
        check_is(O, ix, c.ha, c.dump_a)
        st = ix.stats()
        assert (st["nb_kmers"], st["nb_buckets"]) == c.stats_a
        data, found = ix.lookup(lo, hi, idx)
        assert found.all() and np.array_equal(data, cnt)
        n = 500
        for flip in (np.uint64(1), np.uint64(1) << np.uint64(2 * min(r.k, 32) - 1)):  # the last nucleotide of the k-mer, and one of the first
            lo2 = lo[:n] ^ flip
            want2 = np.array([O.index_get(c.ha, int(a), int(h), int(i)) for a, h, i in zip(lo2, hi[:n], idx[:n])])
            data2, found2 = ix.lookup(lo2, hi[:n], idx[:n])
            assert np.array_equal(found2.astype(bool), want2 >= 0)
            assert np.array_equal(data2[want2 >= 0], want2[want2 >= 0].astype(np.uint8))


@ROWS
def test_index(B, O, tmp_path, r):
    index_family(B, O, tmp_path, r)


# ---- get -----------------------------------------------------------------------------------------------------------------------
def get_family(B, O, tmp_path, r):
    c = G.case(O, r)
    with filled(B, r, tmp_path, c.reads_a) as ix:
        assert np.array_equal(ix.get_reads(c.queries), c.sums)
        check_get_kmers(ix, c, what=G.row_id(r))


@ROWS
def test_get(B, O, tmp_path, r):
    get_family(B, O, tmp_path, r)


# ---- abundance -----------------------------------------------------------------------------------------------------------------
def abundance_family(B, O, tmp_path, r):
    c = G.case(O, r)
    left = keep(c.dump_a, 2, 255)
    assert 10 * len(left[0]) >= len(c.dump_a[0]) and 10 * (len(c.dump_a[0]) - len(left[0])) >= len(c.dump_a[0])
    with filled(B, r, tmp_path, c.reads_a) as ix:
        assert np.array_equal(ix.count_spectrum(), np.bincount(c.dump_a[3], minlength=256).astype(np.uint64))
        got = ix.enumerate(min_count=2, max_count=255)
        assert same_multiset(got, left) and O.digest_entries(*got) == O.digest_entries(*left)
        assert ix.prune(2, 255) == len(c.dump_a[0]) - len(left[0])
        check_is(O, ix, c.ha, left)
        slots, alts = G.filtered_slots(c, 2, 255)
        check_get_kmers(ix, c, slots, alts, "after the prune")


@ROWS
def test_abundance(B, O, tmp_path, r):
    abundance_family(B, O, tmp_path, r)


# ---- set operations --------------------------------------------------------------------------------------------------------------
def set_operations_family(B, O, tmp_path, r):
    c = G.case(O, r)
    for op, rule in (("merge", "left"), ("subtract", "left"), ("intersect", "min"), ("intersect", "sum")):
        want = expected(op, c.da, c.db, rule)
        with filled(B, r, tmp_path, c.reads_a) as ix, filled(B, r, tmp_path, c.reads_b) as src:
            src_before, src_cs = src.enumerate(), src.checksum()
            assert src_cs == O.digest_entries(*as_dump(c.db))
            n = ix.merge(src) if op == "merge" else ix.subtract(src) if op == "subtract" else ix.intersect(src, count=rule)
            assert n == abs(len(want) - len(c.da)), (op, rule)
            check_is(O, ix, c.ha, as_dump(want))
            assert src.checksum() == src_cs and all(np.array_equal(x, y) for x, y in zip(src.enumerate(), src_before)), (op, rule)
            ix.insert_reads(c.reads_c)  # and the index takes inserts afterwards
            check_is(O, ix, c.ha, as_dump(expected("merge", want, c.dc)))
    with filled(B, r, tmp_path, c.reads_a) as a, filled(B, r, tmp_path, c.reads_b) as b:
        assert a.compare(b) == expected_compare(c.da, c.db)
        assert b.compare(a) == expected_compare(c.db, c.da)


@ROWS
def test_set_operations(B, O, tmp_path, r):
    set_operations_family(B, O, tmp_path, r)


# ---- snapshot ----------------------------------------------------------------------------------------------------------------------
def snapshot_family(B, O, tmp_path, monkeypatch, r):
    c = G.case(O, r)
    hab = oracle_index(O, c.reads_a + c.reads_b, r.k, r.m, r.b)  # the oracle index that received A, then B
    want_ab = O.index_dump(hab)
    slots_ab, alts_ab, _ = expected_all(O, hab, c.queries, r.k, r.m)
    path = tmp_path / "a.snap"
    with filled(B, r, tmp_path, c.reads_a) as ix:
        monkeypatch.setenv("BRISK_SNAPSHOT_BLOCK", "1500")  # read at each save: several blocks
        assert ix.save(path) == len(c.dump_a[0])
        monkeypatch.delenv("BRISK_SNAPSHOT_BLOCK")
        lay = ix.layout
    L = G.row_layout(r)
    hdr, blocks = snapshot_reader.read(path)
    assert len(blocks) >= 3 and hdr["n_blocks"] == len(blocks)
    assert (hdr["k"], hdr["m"], hdr["b"], hdr["key_words"], hdr["shift"], hdr["part_bits"]) == (r.k, r.m, r.b, L["key_words"], L["shift"], L["part_bits"])
    assert hdr["n_entries"] == len(c.dump_a[0]) and tuple(hdr["checksum"]) == O.digest_entries(*c.dump_a)
    # the file itself, read by the independent reader, must yield the oracle's entries: every stored key is
    # [bucket's low `shift` bits | compacted k-mer | idx'] of an element of the oracle's records of A, with that element's count,
    # in a partition whose number is the rest of its routing id (bucket, and the class of minimizer_idx where there are classes).
    # (A key alone is not an identity: with shift = 0 the routing id lives in the partition number only, and at k12 m5 b1 entries
    # of different partitions share a key.)
    parts = np.concatenate([bk["partitions"] for bk in blocks])
    assert len(np.unique(parts)) == len(parts) == hdr["n_partitions"] and int(parts.max()) < (1 << L["part_bits"])
    assert all(int(bk["counts"].sum()) == len(bk["keys"]) == len(bk["data"]) for bk in blocks)
    assert G.file_entries(blocks, L) == G.expected_file_entries(O, c, L)
    for room in (False, True):
        with B.BriskHip(r.k, r.m, r.b, **G.opts(r)) as ld:
            assert ld.layout == lay
            assert ld.load(path, room=room) == len(c.dump_a[0])
            check_is(O, ld, c.ha, c.dump_a)
            check_get_kmers(ld, c, what=("loaded", room))
            ld.insert_reads(c.reads_b)  # the loaded index grows
            check_is(O, ld, hab, want_ab)
            assert np.array_equal(ld.get_reads(c.queries), O.index_query_reads(hab, c.qflat, c.qoffs))
            check_get_kmers(ld, c, slots_ab, alts_ab, ("loaded, then grown", room))
    with B.BriskHip.open(path) as ld:  # and the handle that the header alone describes
        assert ld.layout == lay and ld.checksum() == O.digest_entries(*c.dump_a)
    O.index_free(hab)


@ROWS
def test_snapshot(B, O, tmp_path, monkeypatch, r):
    snapshot_family(B, O, tmp_path, monkeypatch, r)


# ---- profiles and extraction ----------------------------------------------------------------------------------------------------------
def profiles_and_extraction_family(B, O, tmp_path, r):
    """The oracle's slots reduced by profile_from_slots are the expected records.  Where a span of a read is its own reverse
    complement the oracle allows two orders of the span's slots (test_kmer_query.expected_slots); get_kmers must return one of
    the two, and the profile, the intervals and the extraction are then held to that one (geometry_edges.resolved_slots): the
    low-complexity reads are checked whole like every other read."""
    import torch
    from extract_reference import pack_reads
    from extract_worker import OutBuffers
    c = G.case(O, r)
    k = r.k
    assert c.clean.mean() > 0.8  # (reads with such spans are among the queries of fourteen rows: test_geometry_edges_cpu.py)
    rules = (B.select_rule("solid_run"), B.select_rule("median", lo=3, hi=255, min_len=90), B.select_rule("present", lo=0, hi=950))
    with filled(B, r, tmp_path, c.reads_a) as ix:
        got_counts, got_found, base = ix.get_kmers(c.queries)
        got_slots = as_u16(got_counts, got_found)
        assert_slots(got_slots, c.slots, c.alts, G.row_id(r))
        slots = G.resolved_slots(c, got_slots)
        assert np.array_equal(slots[~c.ambiguous], c.slots[~c.ambiguous])
        counts, found = (slots & 0xff).astype(np.uint8), (slots & 0x100) != 0
        for solid_min in (1, 2, 256):
            want = B.profile_from_slots(counts, found, c.base, solid_min)
            got = ix.read_profile(c.queries, solid_min)
            assert np.array_equal(got, want), (solid_min, np.nonzero(got != want)[0][:5])
            either = B.profile_from_slots((c.slots & 0xff).astype(np.uint8), (c.slots & 0x100) != 0, c.base, solid_min)
            for f in ORDER_FREE:  # and what no order changes is the oracle's first answer as well
                assert np.array_equal(got[f], either[f]), (solid_min, f)
        want = B.profile_from_slots(counts, found, c.base, 2)
        seqs = c.queries
        words, starts = pack_reads(seqs)
        d_packed, d_starts = torch.from_numpy(words.view(np.int32)).cuda(), torch.from_numpy(starts.view(np.int64)).cuda()
        for rule in rules:
            ivs = B.intervals_from_profile(want, k, rule)
            assert 0 < (ivs["len"] > 0).sum() < len(ivs), rule.kind  # the rule keeps some reads and drops some
            assert np.array_equal(ix.trim_reads(seqs, 2, rule), ivs), rule.kind
            # trim_packed, then unpack_ascii: the Python slices, back to back
            kept = [(i, s[int(v["start"]):int(v["start"]) + int(v["len"])]) for i, (s, v) in enumerate(zip(seqs, ivs)) if v["len"]]
            out = OutBuffers(len(seqs), len(words))
            n_out, n_nts = ix.trim_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), out.packed.data_ptr(), out.cap, out.starts.data_ptr(), out.index.data_ptr(), 2, rule)
            assert (n_out, n_nts) == (len(kept), sum(len(s) for _, s in kept)), rule.kind
            _, o_starts, o_index = out.host()
            assert o_index[:n_out].tolist() == [i for i, _ in kept]
            assert o_starts[:n_out + 1].tolist() == np.concatenate(([0], np.cumsum([len(s) for _, s in kept]))).tolist()
            d_text = torch.zeros(n_nts + 8, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ix.unpack_ascii(out.packed.data_ptr(), 0, n_nts, d_text.data_ptr())
            ix.sync()
            assert d_text.cpu().numpy()[:n_nts].tobytes().decode() == "".join(s for _, s in kept), rule.kind


@ROWS
def test_profiles_and_extraction(B, O, tmp_path, r):
    profiles_and_extraction_family(B, O, tmp_path, r)


# ---- saturating counts -------------------------------------------------------------------------------------------------------------------
def saturating_counts_family(B, O, tmp_path, r, part=None):
    """tests/test_saturate.py's construction -- a read set whose oracle counts are exact, inserted twice -- with one read 300 times
    among it, and a merge whose sums cross 255 between counts that have not.  part: "insert" or "merge" alone (the second handle is
    opened for the merge only), None: both"""
    import saturate_worker as S
    reads, other, one = G.saturate_reads()
    want_a, want_b, nb_a, nb_union = G.saturate_expectation(O, r)
    assert any(v == 255 for v in want_a.values()) and any(v < 255 for v in want_a.values())
    shared = set(want_a) & set(want_b)
    assert any(want_a[x] + want_b[x] > 255 and want_a[x] < 255 and want_b[x] < 255 for x in shared)
    with B.BriskHip(r.k, r.m, r.b, count_mode="saturate", **G.opts(r)) as dst:
        G.check_library_layout(r, dst.layout)
        for batch in (reads, one * 300, reads):  # the filler, the read past 255, the filler again: three calls
            dst.insert_reads(batch)
        if part != "merge":
            S.check_index(dst, want_a, nb_a, r.k, "saturating insert")
            path = tmp_path / "sat.snap"
            dst.save(path)
            info = B.snapshot_info(path)
            G.check_library_layout(r, dst.layout, info)
            assert info["count_mode"] == 1
        if part == "insert":
            return
        with B.BriskHip(r.k, r.m, r.b, count_mode="saturate", **G.opts(r)) as src:
            src.insert_reads(other * 2)
            src_cs = src.checksum()
            merged = {x: S.clamp(want_a.get(x, 0) + want_b.get(x, 0)) for x in set(want_a) | set(want_b)}
            assert dst.merge(src) == len(set(want_b) - set(want_a))
            S.check_index(dst, merged, nb_union, r.k, "saturating merge")
            assert src.checksum() == src_cs and dst.count_spectrum()[0] == 0


@pytest.mark.parametrize("r", [G.TABLE[i] for i in G.SATURATE_ROWS], ids=[G.row_id(G.TABLE[i]) for i in G.SATURATE_ROWS])
def test_saturating_counts(B, O, tmp_path, r):
    saturating_counts_family(B, O, tmp_path, r)


# ---- kernel variants and BRISK_CLS_BITS: a process per environment (the library reads these variables once) ----------------------------
def _worker(mode, extra_env, tmp_path, *more):
    env = {n: v for n, v in os.environ.items() if not n.startswith("BRISK_") or n == "BRISK_HIP_LIB"}
    env.update(extra_env, GEOMETRY_WORKER_DIR=str(tmp_path))
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(TESTS, "geometry_edges_worker.py"), mode, *more], env=env, capture_output=True, text=True, timeout=600)
    print(f"geometry_edges_worker {mode} {extra_env}: {time.time() - t0:.0f} s")
    print(p.stdout)
    last = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
    assert p.returncode == 0 and last.startswith("ok "), (extra_env, p.stdout[-4000:], p.stderr[-6000:])
    return int(last.split()[1])


@pytest.mark.parametrize("env", [{"BRISK_BINS": "2"}, {"BRISK_BINS": "64"}, {"BRISK_BINS": "0", "BRISK_HUGE_AT": "24", "BRISK_HUGE_QUERY_AT": "0"},
                                 {"BRISK_BINS": "0", "BRISK_DEFER": "0"}], ids=["bins-2", "bins-64", "huge", "bins-0-immediate"])
def test_kernel_variants(env, tmp_path):
    """insert in two batches, get_reads, get_kmers and a merge at every row, on the binned record layouts and the
    workgroup-per-partition bodies: tests/geometry_edges_worker.py variants"""
    assert _worker("variants", env, tmp_path) == 5 * len(G.TABLE)


@pytest.mark.parametrize("bits", [0, 2, 3])
def test_cls_bits(B, O, tmp_path, bits):
    """BRISK_CLS_BITS changes where the scan cuts records: index, gets and the records themselves at the class rows, in a child; a
    snapshot saved under one setting is refused under another, both ways round: the child refuses this process's files, this process
    the child's."""
    rows = G.cls_rows()
    mine = {}
    for r in rows:
        c = G.case(O, r)
        with B.BriskHip(r.k, r.m, r.b) as ix:
            ix.insert_reads(c.reads_a)
            mine[r] = ix.layout["cls_bits"]
            ix.save(tmp_path / ("parent-%s.snap" % G.row_id(r)))
    assert _worker("cls", {"BRISK_CLS_BITS": str(bits)}, tmp_path) == 7 * len(rows)
    for r in rows:
        path = tmp_path / ("child-%s.snap" % G.row_id(r))
        assert B.snapshot_info(path)["cls_bits"] == bits
        with B.BriskHip(r.k, r.m, r.b) as ix:
            if mine[r] == bits:
                assert ix.load(path) == len(G.case(O, r).dump_a[0])
                continue
            with pytest.raises(B.BriskHipError) as e:
                ix.load(path)
            assert e.value.code == EINVAL and any(f in str(e.value) for f in ("part_bits", "ext_bits", "cls_bits")), str(e.value)
            assert ix.checksum() == (0, 0, 0)
