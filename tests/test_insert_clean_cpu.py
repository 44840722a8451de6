"""CPU: the read sets of tests/test_insert_clean.py are what that test needs them to be (tests/insert_clean_reads.py; the oracle only),
and the core -- the nucleotides every k-mer window of the fold's common frame covers -- lies where k_insert_first's mask puts it.

CLEAN = partitions k_insert_first takes in which no two records that survive the fold meet (same bucket, intersecting idx' ranges,
same core) and the fold needs at most 16 heads: the table-free path must take them.  Every other partition holds a pair the fold
cannot tell apart from one that shares k-mers, or records it never compared: the probe table must take it.  The GPU test asserts
CLEAN <= table-free <= CLEAN + AMBIG per set; AMBIG is 0 here (the outcome does not hang on the order of arrival)."""
import numpy as np
import pytest

import oracle
import insert_clean_reads as R


@pytest.fixture(scope="module")
def O():
    oracle.build(ref=False)
    return oracle.Oracle()


@pytest.fixture(scope="module")
def censuses(O):
    return {name: R.census(O, R.get(name)) for name in R.SETS}


def test_the_core_lies_in_every_window_of_the_frame():
    # the k-mer of idx' t is the frame's nucleotides [E - 1 - t, E - 1 - t + k - b); idx' runs over [suff_reduc, suff_reduc + k - m]
    assert (R.K, R.M, R.B, R.SUFF, R.E, R.KB) == (63, 21, 14, 4, 47, 49)
    windows = [(R.E - 1 - t, R.E - 1 - t + R.KB) for t in range(R.SUFF, R.SUFF + R.K - R.M + 1)]
    assert (max(a for a, _ in windows), min(b for _, b in windows)) == R.CORE_NT == (42, 49)
    assert R.CORE == ((1 << 14) - 1) << 84  # bits [20, 34) of the frame's second 64-bit word: m - b = 7 nucleotides
    assert R.CORE >> 64 == ((1 << 14) - 1) << 20 and R.CORE & ((1 << 64) - 1) == 0


def _frames(O, reads):
    h = O.index_new(R.K, R.M, R.B)
    try:
        out = []
        for r in reads:
            c, bucket, n, idx0 = O.records(h, r, R.K, R.M, R.B)
            assert len(n) == 1
            big = sum(int(w) << (64 * t) for t, w in enumerate(c[0]))
            out.append((int(bucket[0]), int(idx0[0]), int(n[0]), big << (2 * (R.E - int(idx0[0]) - int(n[0])))))
        return out
    finally:
        O.index_free(h)


def test_the_core_is_the_minimizer_s(O):
    """copies of one centre with other flanks have one core, whole or in part; two centres of one bucket have different cores"""
    cr = R.Crafter(7)
    try:
        part = cr.partition()
        one = cr.copies(part, 1)[0]
        same = [one, R.sub(one, 0, 20), R.sub(one, 0, 42)]
        centre = one[R.K - R.M:R.K]
        while len(same) < 6:
            c = R.R3._copy(O, cr.rng, centre)
            if c is not None:
                same.append(c)
        two = cr.copies(part, 2, bucket=part * 16 + 3)
    finally:
        cr.close()
    fs = _frames(O, same)
    assert len({f[0] for f in fs}) == 1 and len({f[3] & R.CORE for f in fs}) == 1, fs
    assert len({f[3] for f in fs[3:]}) == 3  # (other flanks: other strings)
    a, b = _frames(O, two)
    assert a[0] == b[0] == part * 16 + 3 and (a[3] ^ b[3]) & R.CORE, (a, b)


def test_the_clean_sets_are_clean_at_the_slot_boundaries(censuses):
    for name in ("once", "folds"):
        c = censuses[name]
        assert c["partitions"] == c["LEAN"] == c["CLEAN"] == 30 and c["AMBIG"] == 0, (name, c)
        assert all(c["sizes"].count(s) == 6 for s in R.SIZES), (name, c["sizes"])
    st = censuses["once"]["states"].values()
    assert all(s["records"] == s["survivors"] for s in st)  # every k-mer once: nothing folds
    st = censuses["folds"]["states"].values()
    assert all(s["records"] == s["survivors"] + 3 for s in st)  # two contained reads and one identical copy fold


def test_two_loci_of_one_bucket_are_clean(censuses):
    c = censuses["loci"]
    assert c["partitions"] == c["CLEAN"] == 14 and c["sizes"] == [2 * R.W1] * 14, c


def test_the_table_set_has_nothing_clean(censuses):
    c = censuses["table"]
    assert c["partitions"] == c["LEAN"] == 28 and c["CLEAN"] == 0 and c["AMBIG"] == 0, c
    kinds = sorted((s["records"], s["survivors"], s["instances"]) for s in c["states"].values())
    # overlap: 2 x 30; substitution: 2 x 43; chain: 3 x 16; both sides: 24 + 12 + 20; heads: 18 x 4, all of them survivors
    assert kinds == [(2, 2, 60)] * 8 + [(2, 2, 86)] * 8 + [(3, 3, 48)] * 4 + [(3, 3, 56)] * 4 + [(18, 18, 72)] * 4, kinds
    assert R.FOLD_TRIPS < 18


def test_the_mixed_set_has_more_clean_than_not(censuses):
    c = censuses["mixed"]
    assert c["partitions"] == c["LEAN"] == 34 and c["CLEAN"] == 20 and c["AMBIG"] < c["CLEAN"], c


def test_shared_kmers_count_twice(O):
    """the oracle's counts of one overlap partition and one substitution partition: some k-mers twice, some once"""
    cr = R.Crafter(9)
    try:
        over = R._spans(cr, [(0, 30), (13, 30)])
        subst = R._subst(cr)
    finally:
        cr.close()
    for reads, twice, once in ((over, 17, 26), (subst, None, None)):
        lines = O.count([r.decode() for r in reads], R.K, R.M, R.B)[0]
        cnt = np.array([int(l.split()[2]) for l in lines])
        assert set(cnt.tolist()) == {1, 2}
        if twice is not None:
            assert ((cnt == 2).sum(), (cnt == 1).sum()) == (twice, once)
        else:
            assert (cnt == 2).sum() + (cnt == 1).sum() // 2 == R.W1 and (cnt == 1).sum() % 2 == 0


def test_the_hot_partition_is_left_over(O):
    c = R.census(O, R._pack(R.hot_reads(300)))
    hot = [s for s in c["states"].values() if s["records"] > 64]
    assert len(hot) == 1 and hot[0]["records"] == 302 and not hot[0]["lean"] and hot[0]["survivors"] == 2, hot
    assert c["partitions"] == 13 and c["LEAN"] == c["CLEAN"] == 12, c
