"""CPU: the grouped fold rule of k_insert_first gives what the sequential rule gives (DESIGN.md section 4 finding 21).

tests/fold_group_rules.py restates both rules of brisk_insert.hip -- fold_records (one head per round) and fold_records_grouped
(the head of every slot per round, the sequential rule behind it for more than 16 heads) -- over records in the kernel's frame.
Here: the same (folded, lead, off) per record and the same `clean` per partition on random partitions at working density, on
partitions built over a synthetic locus model (no oracle needed: strings, ranges and core keys are made directly), and on the
crafted sets of the GPU test, whose kinds are checked to be what tests/insert_fold_groups_worker.py says."""
import random

import pytest

import oracle
import insert_clean_reads as R
import fold_group_rules as G
import insert_fold_groups_worker as W


def rec(locus, a, n, bucket=None):
    """the record over k-mers [a, a + n) of synthetic locus `locus`: a 105-nt string whose core is made of the locus number"""
    rng = random.Random(locus)
    full = rng.getrandbits(2 * (R.KB + R.W1 - 1))          # the compacted string of the whole super-k-mer, frame-aligned
    core = locus & ((1 << G.CORE_BITS) - 1)
    full = (full & ~R.CORE) | (core << (2 * R.CORE_NT[0]))
    i0, end = R.SUFF + a, R.SUFF + a + n
    lo = 2 * (R.E - end)
    c = (full >> lo) & ((1 << (2 * (n + R.KB - 1))) - 1)
    return ((locus >> G.CORE_BITS) & 15 if bucket is None else bucket, i0, n, c)


def both(recs):
    fr = G.frames(recs)
    s, g = G.sequential(fr), G.grouped(fr)
    assert (g[0], g[1]) == (s[0], s[1]), (recs, s, g)
    return s, g


def test_slot_hash_is_six_bits_and_spreads():
    slots = [G.slot(ck) for ck in range(1 << 12)]
    assert min(slots) == 0 and max(slots) == 63 and G.slot(0) == 0
    assert G.slot(1) == (0x9E3779B1 >> 26)


@pytest.mark.parametrize("seed", range(4))
def test_random_partitions_at_working_density(seed):
    rng = random.Random(seed)
    rounds = [0, 0]
    for _ in range(400):
        loci = [rng.randrange(1 << 18) for _ in range(rng.choice((1, 2, 3, 4, 4, 5, 8)))]
        recs = []
        for _ in range(rng.choice((3, 8, 12, 13, 16, 30, 64))):
            a = rng.randrange(0, R.W1)
            recs.append(rec(rng.choice(loci), a, rng.randrange(1, R.W1 - a + 1)))
        s, g = both(recs)
        rounds[0] += s[2]
        rounds[1] += g[2]
    assert rounds[1] < rounds[0]


@pytest.mark.parametrize("heads", [1, 2, 16, 17])
def test_partitions_of_so_many_heads(heads):
    # one head per group
    recs = [r for l in range(heads) for r in (rec(1000 + l, 0, 8), rec(1000 + l, 0, 8), rec(1000 + l, 3, 3))]
    s, g = both(recs)
    assert sum(not f for f, _, _ in s[0]) == min(heads, 16) + 3 * max(heads - 16, 0)  # (past the 16th head nothing folds)
    assert g[4] == (heads > 16) and s[1] == (heads <= 16) and (g[4] or g[2] <= s[2])
    # all heads in one group: disjoint two-k-mer reads of one locus, each with a copy
    recs = [r for h in range(heads) for r in (rec(77, 2 * h, 2), rec(77, 2 * h, 2))]
    s, g = both(recs)
    assert sum(not f for f, _, _ in s[0]) == min(heads, 16) + 2 * max(heads - 16, 0) and g[4] == (heads > 16) and s[1] == (heads <= 16)
    assert g[4] or g[2] == heads == s[2]


def test_two_groups_in_one_slot():
    a = 5
    b = next(x for x in range(6, 1 << 14) if G.slot(x) == G.slot(a))
    recs = [rec(a, 0, 43), rec(b, 0, 43), rec(a, 5, 12), rec(b, 7, 9)]
    s, g = both(recs)
    assert g[2] == 2 and g[3] == 2 and not g[4] and s[1]
    assert s[0] == [(False, 0, 0), (False, 1, 0), (True, 0, 5), (True, 1, 7)]


def test_identical_records_and_one_record_per_group():
    s, g = both([rec(9, 4, 20)] * 64)
    assert g[2] == 1 and s[1] and s[0][0] == (False, 0, 0) and all(r == (True, 0, 0) for r in s[0][1:])
    s, g = both([rec(100 + l, 0, 3) for l in range(64)])   # 64 heads: the sequential rule, not clean
    assert g[4] and not s[1] and not any(f for f, _, _ in s[0])


def test_an_unsure_record_hands_the_partition_to_the_sequential_rule():
    recs = [rec(5, 0, 43), (5 >> G.CORE_BITS, R.SUFF - 1, 3, 12345), rec(5, 5, 12)]
    s, g = both(recs)
    assert g[4] and not s[1]


@pytest.fixture(scope="module")
def states():
    oracle.build(ref=False)
    O = oracle.Oracle()
    return {name: list(W.rules_census(O, W.get(name)).values()) for name in W.SETS}


def test_crafted_sets_are_what_they_claim(states):
    for count in (1, 2, 16, 17):
        for s in states[f"groups-{count}"]:
            assert (s["records"], s["groups"], s["instances"], s["lean"]) == (3 * count, count, 8 * count + 11 * max(count - 16, 0), True), s  # (the 17th group stays unfolded)
            assert s["clean"] == (count <= 16) and s["fell_back"] == (count > 16) and s["seq_rounds"] == min(count, 16), s
            assert s["fell_back"] or (s["rounds"] == 1 if s["slots"] == count else s["rounds"] <= count), s
    for s in states["slot"]:
        assert (s["groups"], s["slots"], s["rounds"], s["heads"], s["clean"]) == (2, 1, 2, 2, True), s
    for s in states["chain"]:
        assert (s["groups"], s["heads"], s["clean"], s["lean"]) == (2, 4, False, True) and s["rounds"] >= 3, s
    for s in states["twoheads"]:
        assert (s["records"], s["heads"], s["instances"], s["clean"]) == (3, 2, 40, False), s
    for s in states["rec64"]:
        assert (s["records"], s["heads"], s["instances"], s["clean"]) == (64, 3, 129, True), s
    for s in states["i192"]:
        assert (s["instances"], s["lean"], s["clean"]) == (192, True, True), s
    for s in states["i193"]:
        assert (s["instances"], s["lean"], s["clean"]) == (193, False, False), s
