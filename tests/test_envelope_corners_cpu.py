"""CPU: the corners of brisk_hip_create's parameter envelope (geometry_edges.CORNERS) and the yardstick
itself.  Every corner lays out as its predicate says; its inputs can tell a right answer from a wrong one (the unchanged
non-vacuity conditions of geometry_edges.Case, from the oracle alone); and the restatement (oracle/brisk_oracle.c), which every
device test is compared with, reproduces the reference's own answers at every row of both tables: tests/golden/envelope_reference.json
was written by the reference's sources (tests/golden/make_golden.py envelope), and where oracle/_ref is built the comparison runs
live as well."""
import numpy as np
import pytest

import geometry_edges as G
import oracle
from conftest import load_golden

IDS = [G.row_id(r) for r in G.CORNERS]
ALL = G.all_rows()
ALL_IDS = [G.row_id(r) for r in ALL]


@pytest.mark.parametrize("i", range(len(G.CORNERS)), ids=IDS)
def test_corner_carries_its_property(i):
    r = G.CORNERS[i]
    L = G.row_layout(r)
    assert L is not None
    assert (L["key_bits"], L["key_words"], L["shift"], L["nw"]) == (r.key_bits, r.key_words, r.shift, r.nw), L
    assert L["key_bits"] == L["shift"] + 2 * (r.k - r.b) + 6 <= 128 and L["key_words"] == (1 if L["key_bits"] <= 64 else 2)
    assert L["nw"] == -(-2 * (2 * r.k - r.m - r.b) // 64) and 1 <= L["nw"] <= 4
    assert G.CORNER_PROPERTY[i](L), (r.why, L)
    # the create contract: b <= m < k <= 63, m odd and at most 31, b at most 16, k - b at least 4
    assert 1 <= r.b <= r.m < r.k <= 63 and r.m % 2 == 1 and r.m <= 31 and r.b <= 16 and r.k - r.b >= 4
    assert not r.part_bits and L["part_bits"] <= 27  # 2^30 partitions: every whole enumeration would copy a 4 GiB directory


def test_the_corners_cover_the_edges_of_the_envelope():
    Ls = [G.row_layout(r) for r in G.CORNERS]
    assert len(G.CORNER_PROPERTY) == len(G.CORNERS) == 13 and len(set(G.CORNERS)) == 13 and not set(G.CORNERS) & set(G.TABLE)
    assert len(G.TABLE) == 16 and len(ALL) == 29 and len(set(ALL_IDS)) == 29
    assert {L["b"] for L in Ls} >= {15, 16} and {L["m"] for L in Ls} >= {1, 3, 31}
    assert sum(L["k"] == L["m"] + 1 for L in Ls) >= 2 and sum(L["k"] - L["b"] == 4 for L in Ls) >= 3
    assert any(L["ext_bits"] == L["cls_bits"] == 1 for L in Ls)  # no hash bits left for the routing id
    assert any(L["shift"] == 8 and L["part_bits"] == 24 for L in Ls)  # 256 buckets a partition
    assert {L["nw"] for L in Ls} == {1, 2, 3, 4} and {L["key_words"] for L in Ls} == {1, 2}
    assert max(L["k"] - L["m"] + 1 for L in Ls) == 61
    for rows in (G.SATURATE_CORNERS, G.SHARDED_CORNERS, G.PERCALL_CORNERS):
        assert all(0 <= i < len(G.CORNERS) for i in rows)
    assert [(G.CORNERS[i].k, G.CORNERS[i].m, G.CORNERS[i].b) for i in G.SATURATE_CORNERS] == [(63, 31, 16), (21, 3, 3)]
    assert [(G.CORNERS[i].k, G.CORNERS[i].m, G.CORNERS[i].b) for i in G.SHARDED_CORNERS] == [(63, 31, 16), (31, 15, 15), (63, 3, 2)]
    assert [(G.CORNERS[i].k, G.CORNERS[i].m, G.CORNERS[i].b) for i in G.PERCALL_CORNERS] == [(33, 17, 16), (21, 3, 3)]


@pytest.mark.parametrize("i", range(len(G.CORNERS)), ids=IDS)
def test_inputs_tell_right_from_wrong(O, i):
    """test_geometry_edges_cpu.test_inputs_tell_right_from_wrong over the corners: the same conditions, unchanged"""
    import brisk_amd
    c = G.case(O, G.CORNERS[i])
    fig = c.preconditions()
    print(G.row_id(c.row), fig)
    assert len(c.reads_a) < 1000 and min(len(x) for x in c.reads_a) < c.row.k <= max(len(x) for x in c.reads_a)
    prof = brisk_amd.profile_from_slots((c.slots & 0xff).astype(np.uint8), (c.slots & 0x100) != 0, c.base, 2)
    iv = brisk_amd.intervals_from_profile(prof, c.row.k, brisk_amd.select_rule("solid_run"))[c.clean]
    lens = np.array([len(q) for q, ok in zip(c.queries, c.clean) if ok])
    assert (iv["len"] == 0).any() and (iv["len"] == lens).any() and ((iv["len"] > 0) & (iv["len"] < lens)).any()
    want = G.expected_file_entries(O, c, G.row_layout(c.row))
    assert len(want) == len(c.dump_a[0]) and len({(x[0], x[2]) for x in want}) == len(want)
    assert np.array_equal(np.bincount([x[3] for x in want], minlength=256), np.bincount(c.dump_a[3], minlength=256))
    assert sorted({x[0] for x in want}) == np.unique(O.bucket_ids(c.ha, *c.dump_a[:3])).tolist()
    for rule in (brisk_amd.select_rule("median", lo=3, hi=255, min_len=90), brisk_amd.select_rule("present", lo=0, hi=950)):
        n_kept = int((brisk_amd.intervals_from_profile(prof, c.row.k, rule)["len"] > 0).sum())
        assert 0 < n_kept < len(c.queries), rule.kind
    assert c.clean.mean() > 0.8


def test_bucket_ids_with_bit_31_set_exist(O):
    """b = 16: the routing id fills the 32-bit header field, and the rows' reads reach its upper half; b = 15: bit 29"""
    for i, top in ((0, 31), (1, 31), (2, 31), (5, 31), (3, 29), (4, 29), (6, 29)):
        c = G.case(O, G.CORNERS[i])
        ids = O.bucket_ids(c.ha, *c.dump_a[:3])
        assert c.row.b == (top + 1) // 2 and int(ids.max()) >> top == 1, (G.row_id(c.row), hex(int(ids.max())))
        assert len(np.unique(ids >> 8)) > 100  # and over many partitions


@pytest.mark.parametrize("i", G.SATURATE_CORNERS, ids=[IDS[i] for i in G.SATURATE_CORNERS])
def test_saturating_inputs_cross_255(O, i):
    want_a, want_b, _, _ = G.saturate_expectation(O, G.CORNERS[i])
    shared = set(want_a) & set(want_b)
    assert any(want_a[x] + want_b[x] > 255 and want_a[x] < 255 and want_b[x] < 255 for x in shared)
    assert any(v == 255 for v in want_a.values()) and any(v < 255 for v in want_a.values())


# ---- the yardstick against the reference's own answers ------------------------------------------------------------------------
def test_the_reference_file_names_every_row():
    ref = load_golden("envelope_reference.json")
    assert sorted(ref) == sorted(ALL_IDS)
    assert all((ref[G.row_id(r)]["k"], ref[G.row_id(r)]["m"], ref[G.row_id(r)]["b"]) == (r.k, r.m, r.b) for r in ALL)
    assert all(v["nb_kmers"] > 5000 and v["nb_buckets"] > 1 for v in ref.values())


@pytest.mark.parametrize("r", ALL, ids=ALL_IDS)
def test_restatement_reproduces_the_reference(O, r):
    """multiset, nb_kmers, nb_buckets and the per-read sums of the row's queries: the restatement's, against what the reference's
    sources answered on the same inputs (rebuilt here from the row's seed)"""
    assert G.envelope_answers(O, r) == load_golden("envelope_reference.json")[G.row_id(r)]


# The reference zero-fills a directory of 4^b buckets per index: 6 s a row at b = 15 and 23 to 39 s at b = 16, against 1 to 3 s below.
# Those seven rows are held to the reference by envelope_reference.json alone, which the same calls wrote.
LIVE = [r for r in ALL if r.b <= 14]


@pytest.mark.skipif(not oracle.have_ref(), reason="oracle/_ref/libbrisk_ref.so is not built (needs the reference tree)")
@pytest.mark.parametrize("r", LIVE, ids=[G.row_id(r) for r in LIVE])
def test_restatement_against_the_reference_build_live(O, r):
    """the same where oracle/_ref is built, and the enumerator stream of the first forty reads with it"""
    R = oracle.Ref()
    assert G.envelope_answers(R, r) == G.envelope_answers(O, r) == load_golden("envelope_reference.json")[G.row_id(r)]
    for s in G.read_sets(r)[0][:40]:
        assert all(np.array_equal(x, y) for x, y in zip(R.enumerate(s, r.k, r.m), O.enumerate(s, r.k, r.m))), s


def test_parameter_contract(O):
    """brisk_hip_create's envelope on the restatement: k - b < 4 is refused (the reference aborts there: SuperKmerLight.hpp:62
    takes Pow2 of 2 (k - b) - 8), k - b = 4 is the shortest compacted k-mer it stores"""
    for k, m, b in ((12, 11, 11), (18, 17, 16), (8, 7, 7), (17, 15, 15), (4, 3, 1), (19, 17, 16), (2, 1, 1), (6, 3, 3),
                    (31, 11, 14), (31, 12, 4), (31, 31, 4), (64, 21, 14), (31, 11, 0), (63, 33, 4)):
        with pytest.raises(ValueError):
            O.index_new(k, m, b)
    for r in ALL:
        assert r.k - r.b >= 4
        O.index_free(O.index_new(r.k, r.m, r.b))
    for k, m, b in ((20, 17, 16), (19, 15, 15), (9, 5, 5), (5, 1, 1), (7, 3, 3)):
        lines, nk, nb = O.count(["ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGGCTAGC"], k, m, b)
        assert nk == len(lines) > 0 and nb > 0
    assert G.layout(12, 11, 11) is None and G.layout(18, 17, 16) is None and G.layout(20, 17, 16) is not None
