"""CPU: the geometry table of tests/geometry_edges.py.  Every row carries the property its last column names, from the Python
restatement of brisk_hip_create's layout formula; and the inputs of tests/test_geometry_edges.py can tell a right answer from a
wrong one -- the non-vacuity conditions, from the oracle alone."""
import numpy as np
import pytest

import geometry_edges as G

IDS = [G.row_id(r) for r in G.TABLE]


@pytest.mark.parametrize("i", range(len(G.TABLE)), ids=IDS)
def test_row_carries_its_property(i):
    r = G.TABLE[i]
    L = G.row_layout(r)
    assert L is not None
    assert (L["key_bits"], L["key_words"], L["shift"], L["nw"]) == (r.key_bits, r.key_words, r.shift, r.nw), L
    assert L["key_bits"] == L["shift"] + 2 * (r.k - r.b) + 6 <= 128 and L["key_words"] == (1 if L["key_bits"] <= 64 else 2)
    assert L["nw"] == -(-2 * (2 * r.k - r.m - r.b) // 64) and 1 <= L["nw"] <= 4
    assert G.PROPERTY[i](L), (r.why, L)
    # the create contract: b <= m < k <= 63, m odd and at most 31, b at most 16
    assert 1 <= r.b <= r.m < r.k <= 63 and r.m % 2 == 1 and r.m <= 31 and r.b <= 16


def test_the_table_covers_every_branch_point():
    Ls = [G.row_layout(r) for r in G.TABLE]
    assert len(G.PROPERTY) == len(G.TABLE) == 16 and len(set(G.TABLE)) == 16
    assert {L["key_bits"] for L in Ls} >= {64, 66, 128} and {L["nw"] for L in Ls} == {1, 2, 3, 4}
    assert sum(L["straddle"] for L in Ls) == 3 and sum(L["adjusted"] > 0 for L in Ls) == 1
    assert {L["k"] for L in Ls} >= {32, 33} and {L["wide_record"] for L in Ls} == {False, True}
    assert {L["cls_bits"] for L in Ls} == {0, 1}
    assert all(G.TABLE[i].key_bits in (64, 66, 128) for i in G.SATURATE_ROWS) and G.row_layout(G.TABLE[G.SATURATE_ROWS[2]])["straddle"]


def test_formula_on_the_geometries_the_other_tests_use():
    """key widths of the seven geometries every feature was tested on before, as DESIGN.md section 4.s lists them"""
    seven = [((63, 21, 14), 0), ((31, 15, 14), 0), ((31, 11, 11), 0), ((47, 13, 8), 0), ((47, 13, 8), 12), ((63, 21, 14), 20), ((47, 13, 8), 4)]
    assert sorted(G.layout(*kmb, part_bits=pb)["key_bits"] for kmb, pb in seven) == [44, 46, 84, 88, 96, 108, 112]
    assert G.layout(63, 21, 14)["shift"] == 4 and G.layout(31, 11, 11)["cls_bits"] == 1 and G.layout(31, 11, 11)["cls_width"] == 11
    assert G.layout(63, 21, 1, part_bits=1) is None  # 1 + 2 * 62 + 6 > 128 and nothing left to give: refused
    for env, bits in ((0, 0), (2, 2), (3, 3), (7, 3)):  # BRISK_CLS_BITS
        L = G.layout(33, 11, 4, cls_env=env)
        assert L["cls_bits"] == bits and L["cls_width"] == ((23 + (1 << bits) - 1) >> bits if bits else 1) and L["ext_bits"] == min(16, 14, 16 - bits) + bits
    assert all(G.row_layout(r)["cls_bits"] == 1 for r in G.CLS_EXTRA)
    # an extended routing id is never cut (ext_bits > 0 => shift == 0): BRISK_CLS_BITS=3 at m = 11, b >= 5 gives 25 routing bits and
    # 2^25 partitions, not 2^24 partitions of two classes each (nb_buckets counted those as two buckets)
    L = G.layout(31, 11, 11, cls_env=3)
    assert (L["ext_bits"], L["part_bits"], L["shift"]) == (3, 25, 0)
    for k, m, b in ((31, 11, 11), (33, 11, 4), (63, 11, 5), (40, 7, 7), (20, 9, 3), (63, 5, 2), (12, 5, 1)):
        for env in (-1, 0, 1, 2, 3):
            L = G.layout(k, m, b, cls_env=env)
            assert L["shift"] == 0 or L["ext_bits"] == 0, (k, m, b, env, L)


@pytest.mark.parametrize("i", range(len(G.TABLE)), ids=IDS)
def test_inputs_tell_right_from_wrong(O, i):
    c = G.case(O, G.TABLE[i])
    fig = c.preconditions()
    print(G.row_id(c.row), fig)
    assert len(c.reads_a) < 1000 and min(len(x) for x in c.reads_a) < c.row.k <= max(len(x) for x in c.reads_a)
    # extraction: the solid-run rule keeps some reads whole, trims some and drops some
    import brisk_amd
    prof = brisk_amd.profile_from_slots((c.slots & 0xff).astype(np.uint8), (c.slots & 0x100) != 0, c.base, 2)
    iv = brisk_amd.intervals_from_profile(prof, c.row.k, brisk_amd.select_rule("solid_run"))[c.clean]
    lens = np.array([len(q) for q, ok in zip(c.queries, c.clean) if ok])
    assert (iv["len"] == 0).any() and (iv["len"] == lens).any() and ((iv["len"] > 0) & (iv["len"] < lens)).any()
    # the snapshot expectation built from the oracle's records is the oracle's index: as many identities, the same counts
    want = G.expected_file_entries(O, c, G.row_layout(c.row))
    assert len(want) == len(c.dump_a[0]) and len({(x[0], x[2]) for x in want}) == len(want)
    assert np.array_equal(np.bincount([x[3] for x in want], minlength=256), np.bincount(c.dump_a[3], minlength=256))
    assert sorted({x[0] for x in want}) == np.unique(O.bucket_ids(c.ha, *c.dump_a[:3])).tolist()
    for rule in (brisk_amd.select_rule("median", lo=3, hi=255, min_len=90), brisk_amd.select_rule("present", lo=0, hi=950)):  # and the whole-read rules
        n_kept = int((brisk_amd.intervals_from_profile(prof, c.row.k, rule)["len"] > 0).sum())
        assert 0 < n_kept < len(c.queries), rule.kind


def test_most_rows_query_reads_whose_slot_order_the_oracle_leaves_open(O):
    """spans that are their own reverse complement (the low-complexity reads): the order-dependent checks of profiles and extraction
    meet them at all but two rows"""
    assert sum(not G.case(O, r).clean.all() for r in G.TABLE) >= 14


@pytest.mark.parametrize("i", G.SATURATE_ROWS, ids=[IDS[i] for i in G.SATURATE_ROWS])
def test_saturating_inputs_cross_255(O, i):
    want_a, want_b, _, _ = G.saturate_expectation(O, G.TABLE[i])
    shared = set(want_a) & set(want_b)
    assert any(want_a[x] + want_b[x] > 255 and want_a[x] < 255 and want_b[x] < 255 for x in shared)
    assert any(v == 255 for v in want_a.values()) and any(v < 255 for v in want_a.values())
