"""CPU: the committed sibling pairs (tests/golden/sibling_pairs.json.gz, written by `python tests/sibling_keys.py`) are what
tests/sibling_keys.py says they are -- from the oracle's records alone -- and there are enough of them: the device tests of
tests/test_sibling_keys.py are vacuous without pairs in every sibling bit of every geometry."""
import pytest

import sibling_keys as S

# pairs per sibling bit (singles, records), multi-bit pairs, pairs on each side of the word boundary
FLOOR_BODY = dict(single=8, record=4, multi=8, side=4)
# The other table rows with shift > 0: the yield was not known when the floor was set, so the floor is one pair per sibling bit.
# Measured with the committed seeds, every one of them fills find_pairs' targets like the rows above -- 8 singles and 4 records per
# sibling bit, 8 + 4 multi-bit pairs -- within the candidates given (of 200 000 allowed):
MEASURED_ROWS = {"k63m21b4-pb1": 1196, "k45m27b14": 1380, "k33m31b14": 974}
REGENERATED = ("k63m21b14-pb26", "k33m11b6-pb6")


@pytest.fixture(scope="module")
def data():
    return S.load_fixture()


def test_fixture_holds_every_geometry(data):
    assert list(sorted(data)) == sorted(S.geo_id(g) for g in S.GEOMETRIES)
    ids = [S.geo_id(g) for g in S.GEOMETRIES]
    for gid in ("k63m21b14", "k63m21b14-pb25", "k63m21b14-pb26", "k63m21b14-pb27", "k31m15b14", "k31m15b14-pb23", "k31m15b14-pb22", "k31m11b11",
                "k33m11b6-pb6", "k37m15b10-pb8", "k31m11b4-pb2", "k63m21b4-pb1", "k45m27b14", "k33m31b14", "k33m11b4", "k34m11b4"):
        assert gid in ids
    # the compile-time bodies' shifts: <3,49,4..1>, <2,17,4..6>, <2,20,0>
    assert [(S.geo_layout(g)["nw"], g.k - g.b, S.geo_layout(g)["shift"]) for g in S.BODIES] == [(3, 49, 4), (3, 49, 3), (3, 49, 2), (3, 49, 1), (2, 17, 4), (2, 17, 5),
                                                                                                  (2, 17, 6), (2, 20, 0)]
    for g in S.GEOMETRIES:
        d = data[S.geo_id(g)]
        assert (d["k"], d["m"], d["b"], d["part_bits"], d["seed"]) == (g.k, g.m, g.b, g.part_bits, S.geo_seed(g))
        assert d["candidates"] < S.LIMIT, (S.geo_id(g), "a target ran out of candidates")
        assert (S.geo_layout(g)["shift"] > 0) == (g.kind != "cousins")


@pytest.mark.parametrize("g", S.GEOMETRIES, ids=[S.geo_id(g) for g in S.GEOMETRIES])
def test_every_pair_is_what_it_claims(O, data, g):
    """both members are one super-k-mer with the same C, n and idx0; siblings differ inside the low `shift` bucket bits and share
    the partition, cousins differ in one bit above them; no read occurs twice"""
    L, pairs = S.geo_layout(g), data[S.geo_id(g)]["pairs"]
    h = O.index_new(g.k, g.m, g.b)
    for p in pairs:
        S.verify_pair(O, h, g, L, p)
    O.index_free(h)
    reads = [p[x] for p in pairs for x in "ab"]
    assert len(set(reads)) == len(reads) and len(set(reads) | {S.revcomp(s) for s in reads}) == 2 * len(reads)


@pytest.mark.parametrize("g", S.GEOMETRIES, ids=[S.geo_id(g) for g in S.GEOMETRIES])
def test_floors(data, g):
    L, pairs = S.geo_layout(g), data[S.geo_id(g)]["pairs"]
    n, words = S.tally(L, pairs)
    shift = L["shift"]
    for size in ("single", "record"):
        assert n.get(("cousin", size, "any"), 0) >= 4, (S.geo_id(g), size, "cousins: the control")
    if g.kind == "cousins":
        assert not any(c == "sibling" for c, _, _ in n)
        return
    strict = g.kind in ("body", "straddle")
    assert strict or S.geo_id(g) in MEASURED_ROWS
    if not strict:
        assert data[S.geo_id(g)]["candidates"] == MEASURED_ROWS[S.geo_id(g)]
    for t in range(shift):
        assert n.get(("sibling", "single", (t,)), 0) >= (FLOOR_BODY["single"] if strict else 1), (S.geo_id(g), "bit", t, n)
        assert n.get(("sibling", "record", (t,)), 0) >= (FLOOR_BODY["record"] if strict else 1), (S.geo_id(g), "bit", t, n)
    if strict and shift >= 2:  # (one sibling bit -- k63 m21 b14 with 2^27 partitions -- has no multi-bit pair)
        assert n.get(("sibling", "single", "multi"), 0) >= FLOOR_BODY["multi"], (S.geo_id(g), n)
        assert n.get(("sibling", "record", "multi"), 0) >= FLOOR_BODY["record"], (S.geo_id(g), n)
    if g.kind == "straddle":
        assert L["straddle"] and L["entry_bits"] < 64 < L["entry_bits"] + shift
        for size in ("single", "record"):
            for side in ("low", "high"):
                assert words.get((size, side), 0) >= FLOOR_BODY["side"], (S.geo_id(g), size, side, words)
        assert sum(words.get((size, "both"), 0) for size in ("single", "record")) >= 1  # and a pair that changes both words
    else:
        assert not words


def test_read_sets(data):
    """what the device tests insert: X holds every unprimed member (singles three times, records twice), Y every primed one once;
    they share 30 background reads"""
    g = S.BODIES[2]
    pairs = data[S.geo_id(g)]["pairs"]
    x, y, bg = S.read_sets(g, pairs)
    assert all(x.count(p["a"]) == (3 if p["size"] == "single" else 2) and y.count(p["b"]) == 1 for p in pairs)
    assert not any(p["b"] in x or p["a"] in y for p in pairs)
    assert len(x) == len(bg) + sum(3 if p["size"] == "single" else 2 for p in pairs) and len(y) == 30 + len(pairs)
    assert (x, y, bg) == S.read_sets(g, pairs)


@pytest.mark.parametrize("g", S.GEOMETRIES, ids=[S.geo_id(g) for g in S.GEOMETRIES])
def test_case_preconditions(O, g):
    """what the device tests rely on, from the oracle alone: the two members of a pair are disjoint sets of identities, X holds one
    and Y the other, and a read of a primed member finds nothing in the oracle's index of X"""
    fig = S.case(O, g).preconditions()
    assert fig["pairs"] >= 12 and fig["entries_x"] > fig["entries_y"] > fig["shared"]


@pytest.mark.parametrize("gid", REGENERATED)
def test_the_fixture_is_what_the_generator_writes(O, data, gid):
    g = next(g for g in S.GEOMETRIES if S.geo_id(g) == gid)
    pairs, tried = S.find_pairs(O, g.k, g.m, g.b, g.part_bits, S.geo_seed(g))
    assert tried == data[gid]["candidates"] and pairs == data[gid]["pairs"]
