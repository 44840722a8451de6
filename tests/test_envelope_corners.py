"""GPU: the corners of brisk_hip_create's parameter envelope (geometry_edges.CORNERS): b = 15 and 16, where
the bucket id fills the 32-bit header field and ids with bit 31 set exist; m = 1 and 3, with the degenerate decycling tables, no
hash bits for the routing id and windows of up to 61 k-mers; k = m + 1; k - b = 4.  The families of tests/test_geometry_edges.py
run over these rows unchanged (the same functions of a row), and so do the sharded, per-call, reallocate and kernel-variant checks
of their own modules.  test_library_reproduces_the_reference holds the library to the reference's own answers
(tests/golden/envelope_reference.json) at every row of both tables, with no restatement in between."""
import random

import numpy as np
import pytest

import geometry_edges as G
import oracle
import test_geometry_edges as E
from conftest import load_golden

pytestmark = pytest.mark.gpu

EINVAL = 1
CORNERS = pytest.mark.parametrize("r", G.CORNERS, ids=[G.row_id(r) for r in G.CORNERS])
ALL = G.all_rows()
pick = lambda rows: pytest.mark.parametrize("r", [G.CORNERS[i] for i in rows], ids=[G.row_id(G.CORNERS[i]) for i in rows])


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


# ---- the families of test_geometry_edges.py ------------------------------------------------------------------------------------------
@CORNERS
def test_index(B, O, tmp_path, r):
    E.index_family(B, O, tmp_path, r)


@CORNERS
def test_get(B, O, tmp_path, r):
    E.get_family(B, O, tmp_path, r)


@CORNERS
def test_abundance(B, O, tmp_path, r):
    E.abundance_family(B, O, tmp_path, r)


@CORNERS
def test_set_operations(B, O, tmp_path, r):
    E.set_operations_family(B, O, tmp_path, r)


@CORNERS
def test_snapshot(B, O, tmp_path, monkeypatch, r):
    E.snapshot_family(B, O, tmp_path, monkeypatch, r)


@CORNERS
def test_profiles_and_extraction(B, O, tmp_path, r):
    E.profiles_and_extraction_family(B, O, tmp_path, r)


# in two halves: at b = 16 every handle carries a 512 MiB bucket bitmap, and the merge needs two of them
@pick(G.SATURATE_CORNERS)
def test_saturating_insert(B, O, tmp_path, r):
    E.saturating_counts_family(B, O, tmp_path, r, "insert")


@pick(G.SATURATE_CORNERS)
def test_saturating_merge(B, O, tmp_path, r):
    E.saturating_counts_family(B, O, tmp_path, r, "merge")


# ---- the reference's own answers, no restatement in between ------------------------------------------------------------------------------
@pytest.mark.parametrize("r", ALL, ids=[G.row_id(r) for r in ALL])
def test_library_reproduces_the_reference(B, r):
    """multiset, nb_kmers, nb_buckets and get_reads of the row's queries against what the reference's sources answered on the same
    inputs (tests/golden/make_golden.py envelope)"""
    want = load_golden("envelope_reference.json")[G.row_id(r)]
    a, b, c = G.read_sets(r)
    with B.BriskHip(r.k, r.m, r.b, **G.opts(r)) as ix:
        ix.insert_reads(a)
        st = ix.stats()
        got = dict(k=r.k, m=r.m, b=r.b, nb_kmers=st["nb_kmers"], nb_buckets=st["nb_buckets"],
                   md5=G.lines_md5(oracle.multiset_lines(*ix.enumerate(), r.k)), sums_md5=G.sums_md5(ix.get_reads(G.queries_of(a, b, c))))
    assert got == want


# ---- kernel variants ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"BRISK_BINS": "2"}, {"BRISK_BINS": "64"}, {"BRISK_BINS": "0", "BRISK_HUGE_AT": "24", "BRISK_HUGE_QUERY_AT": "0"},
                                 {"BRISK_BINS": "0", "BRISK_DEFER": "0"}], ids=["bins-2", "bins-64", "huge", "bins-0-immediate"])
def test_kernel_variants(env, tmp_path):
    """test_geometry_edges.test_kernel_variants' environments over the corners.  At b = 16 a partition holds 256 buckets
    (part_bits = 24, shift = 8): "huge" sends them through the workgroup bodies' bucket-bitmap update."""
    assert E._worker("variants", env, tmp_path, "corners") == 5 * len(G.CORNERS)


# ---- sharded: the owner of a 32-bit, of a 30-bit and of an extended routing id ----------------------------------------------------------
@pick(G.SHARDED_CORNERS)
def test_sharded_count_and_get(B, r):
    import test_sharded
    test_sharded.boundary_geometry(B, r)


@pick(G.SHARDED_CORNERS)
def test_sharded_kmers(B, r):
    import sharded_cases as C
    import sharded_kmers_job as K
    K.check_case(B, C.edge_reads(r), C.edge_queries(r), r.k, r.m, r.b, 3, part_bits=r.part_bits)


# ---- the per-call path ---------------------------------------------------------------------------------------------------------------------
@pick(G.PERCALL_CORNERS)
def test_percall_stream_upsert_find_enumerate(B, O, r):
    """test_percall_edges.test_stream and test_upsert_find_enumerate's checks at two corners"""
    import percall_reference as P
    import test_percall_edges as PE
    rp, what = P.replay(O, r), G.row_id(r)
    lo, hi, idx = rp.arrays()
    with PE.handle(B, r) as ix:
        PE.check_stream(ix, rp, what)
        assert ix.stats()["nb_kmers"] == 0
        assert (ix.find_kmers(lo[:300], hi[:300], idx[:300]) == P.ABSENT).all(), (what, "find_kmers on a fresh handle")
        PE.fill(ix, rp, what)
        PE.check_find_all(ix, rp, what)
        for lo2, hi2, idx2, want in P.flipped(rp, O, r):
            assert np.array_equal(ix.find_kmers(lo2, hi2, idx2), want), (what, "find_kmers of one-bit neighbours")
        PE.check_end_state(O, ix, rp, r, what)


# ---- reallocate from a corner ----------------------------------------------------------------------------------------------------------------
# (k, m, b) of the corners whose (k, m + 2, b + 2) brisk_hip_create accepts: b = 15 and 16 have no target (b + 2 > 16), (9, 5, 5) none
# (k - b would be 2), (16, 15, 7) none (m + 2 > k)
REALLOCATE_SOURCES = [(31, 1, 1), (63, 3, 2), (10, 3, 1), (21, 3, 3)]


def test_reallocate_sources_are_corners_with_a_target():
    """(no device call) every source is a corner, every target lays out, and no other corner has a target"""
    corners = {(r.k, r.m, r.b) for r in G.CORNERS}
    assert set(REALLOCATE_SOURCES) == {x for x in corners if x[1] + 2 < x[0] and x[1] + 2 <= 31 and x[2] + 2 <= 16 and G.layout(x[0], x[1] + 2, x[2] + 2) is not None}
    assert (G.layout(63, 5, 4)["key_bits"], G.layout(31, 3, 3)["key_bits"], G.layout(31, 3, 3)["ext_bits"]) == (124, 62, 1)


@pytest.mark.parametrize("k,m,b", REALLOCATE_SOURCES)
def test_reallocate_from_a_corner(O, k, m, b):
    from test_reallocate import _reallocate_and_check
    # (31, 1, 1): 1500 reads leave 107,000 entries whose largest count is 13 (the oracle's); 400 reads six times each leave 40,000
    # with counts up to 30
    _reallocate_and_check(O, k, m, b, 0, 0, **(dict(times=6, n=400) if m == 1 else {}))


# ---- order keys at the degenerate decycling tables -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,b", [(31, 1, 1), (10, 3, 1), (63, 3, 2)])
def test_order_keys_at_m_1_and_3(B, O, k, m, b):
    """debug_order_keys, the table-driven class against the plain FP64 fold against the oracle: every m-mer there is (4 and 64 of
    them), every zero-padded prefix among them, in a random order long enough for every lane"""
    rng = random.Random(k * 100 + m)
    xs = list(range(1 << (2 * m))) * 3 + [rng.getrandbits(2 * m) for _ in range(20000)]
    want = O.key_many(xs, m)
    assert len(set(want.tolist())) == 1 << (2 * m)  # a key is an m-mer's own
    with B.BriskHip(k, m, b) as ix:
        fast = ix.debug_order_keys(xs)
        exact = ix.debug_order_keys(xs, exact=True)
        assert np.array_equal(fast, exact)
        assert np.array_equal(fast, want)
