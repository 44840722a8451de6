"""The arithmetic behind the scan's order-key evaluation, restated in numpy and held against plain restatements of what it replaces.
No device: what holds here is what the kernels in brisk_scan.hip compute with (the device side is test_scan_keys.py)."""
import random

import numpy as np
import pytest

import scan_keys_inputs as SK

U = np.uint64
AA = U(0xAAAAAAAAAAAAAAAA)
MS = (13, 15, 19, 21, 27, 31)


def rev_nts64(x):
    """the order of the 32 nucleotides of a 64-bit value reversed"""
    x = np.asarray(x, U)
    out = np.zeros_like(x)
    for j in range(32):
        out |= ((x >> U(2 * j)) & U(3)) << U(2 * (31 - j))
    return out


def rc_plain(x, n):
    """true reverse complement of an n-mer (rcbc, Kmers.cpp:320-332): nucleotide j, complemented (code ^ 2), to position n-1-j"""
    x = np.asarray(x, U)
    out = np.zeros_like(x)
    for j in range(n):
        out |= (((x >> U(2 * j)) & U(3)) ^ U(2)) << U(2 * (n - 1 - j))
    return out


def low_values():
    rs = np.random.RandomState(20240)
    rnd = rs.randint(0, 1 << 32, 10000).astype(U) << U(32) | rs.randint(0, 1 << 32, 10000).astype(U)
    p3 = [SK.mmer((u * 32)[:32]) for u in ("ACG", "CGA", "GAC", "AAT", "TTA", "AGT", "CCG")]
    p2 = [0x5555555555555555, 0xAAAAAAAAAAAAAAAA, SK.mmer("AC" * 16), SK.mmer("GT" * 16)]
    edge = [0, 0xFFFFFFFFFFFFFFFF, SK.mmer("T" * 32), SK.mmer("A" * 12 + "ACGTTGCAGGTCATTGACCA"), 1, 1 << 63, 3 << 62]
    return np.concatenate([rnd, np.array(p3 + p2 + edge, U)])


@pytest.mark.parametrize("m", MS)
def test_rc_slice_identity(m):
    """Window wl of a k-mer's low 64 bits is (low >> 2 wl) & M, zero-padded where it sticks out of them.  Its reverse complement is a
    slice of one 64-bit value per k-mer, in the form the kernel uses (V = the reversal of low; one left and one right shift, of which
    one is 0; the complement after the shift) and in the form of the reverse complement R = rc64(low, 32) with the 0xAA.. fill."""
    low = low_values()
    M = U((1 << (2 * m)) - 1)
    V = rev_nts64(low)
    R = rc_plain(low, 32)
    assert np.array_equal(R, V ^ AA)
    for wl in range(32):
        want = rc_plain((low >> U(2 * wl)) & M, m)
        c2, wl2 = 2 * (32 - m), 2 * wl
        sr, sl = max(c2 - wl2, 0), max(wl2 - c2, 0)
        got = (((V << U(sl)) >> U(sr)) ^ AA) & M
        assert np.array_equal(got, want), (m, wl)
        if wl <= 32 - m:
            got_r = (R >> U(2 * (32 - m - wl))) & M
        else:
            e2 = 2 * (wl - (32 - m))
            got_r = ((R << U(e2)) & M) | (AA & U((1 << e2) - 1))
        assert np.array_equal(got_r, want), (m, wl)


def test_class_decode_small_and_full_range():
    """The biased unsigned decode against the plain signed comparisons: every (a, b) in [-64, 64]^2 -- both thresholds, both signs,
    the borrow at a < 0 -- and 10^6 seeded pairs over the whole range of a sum."""
    g = np.arange(-64, 65, dtype=np.int64)
    a, b = [v.ravel() for v in np.meshgrid(g, g)]
    rs = np.random.RandomState(77)
    lim = (1 << 31) - 1
    ra, rb = rs.randint(-lim, lim + 1, 1000000, dtype=np.int64), rs.randint(-lim, lim + 1, 1000000, dtype=np.int64)
    # and large sums beside small ones, which the pairs above practically never hold
    small = rs.randint(-40, 41, 1000000, dtype=np.int64)
    for x, y in ((a, b), (ra, rb), (ra, small), (small, rb)):
        cp, gp = SK.decode_plain(x, y)
        cb, gb = SK.decode_biased(x, y)
        assert np.array_equal(gp, gb)
        assert np.array_equal(cp[~gp], cb[~gb])  # (inside the band the class is not used: the exact fold decides)
        assert np.array_equal(cp, cb)
    # a sum that is exactly 0 is never in the band, whatever the other one is outside it
    z = np.zeros(4, np.int64)
    assert not SK.decode_biased(z, np.array([0, 5, -12, 1 << 30]))[1].any()
    assert not SK.decode_biased(np.array([0, -5, 12, -(1 << 30)]), z)[1].any()


@pytest.mark.parametrize("m", (11, 15, 19, 21))
def test_table_sums_bound_and_low_complexity(O, m):
    """The rounded tables' sums stay within 4 units of the exact sums (what the thresholds are built on), and homopolymers and the
    m-mers of period 2 and 3 -- sums of exactly 0 among them -- stay out of the guard band."""
    coef = O.coef_table(m)
    rs = np.random.RandomState(m)
    xs = (rs.randint(0, 1 << 31, 1 << 16).astype(U) << U(31) | rs.randint(0, 1 << 31, 1 << 16).astype(U)) & U((1 << (2 * m)) - 1)
    xs = np.concatenate([xs, np.array(SK.periodic_mmers(m), U)])
    A, B = SK.table_sums(xs, m, coef)
    r, rr = SK.fold_sums(xs, m, coef)
    assert np.max(np.abs(A - np.ldexp(r, 24))) <= 4 and np.max(np.abs(B - np.ldexp(rr, 24))) <= 4
    assert max(np.max(np.abs(A)), np.max(np.abs(B))) < 1 << 30
    per = np.array(SK.periodic_mmers(m), U)
    assert not SK.decode_biased(*SK.table_sums(per, m, coef))[1].any()
    # outside the band the integer class is the reference's
    cls, guard = SK.decode_biased(A, B)
    want = O.class_many([int(x) for x in xs], m)
    assert np.array_equal(cls[~guard], np.asarray(want)[~guard])


def test_band_mmers_are_in_the_band(O):
    """m = 19 has m-mers inside the guard band; the device test counts on these."""
    m = 19
    coef = O.coef_table(m)
    xs = SK.band_mmers(m, coef, 5)
    assert len(xs) == 64
    assert SK.decode_biased(*SK.table_sums(xs, m, coef))[1].sum() == 64


@pytest.mark.parametrize("m,some", ((11, False), (15, False), (21, False), (19, True)))
def test_which_m_have_an_mmer_in_the_guard_band(O, m, some):
    """Over ALL m-mers: at m = 11, 15 and 21 neither sum comes anywhere near the band -- nothing between 8 and 25 units (the band's
    13..20 widened by the 4 units the tables' rounding can take, and one more) --, so the exact fold behind the guard branch never
    runs at the geometries with compile-time bodies and the device test cannot ask for it there; m = 19 has such m-mers.  Should
    CLS_W, the thresholds or the unit change, this is where it shows."""
    nr, nrot = SK.count_band_mmers(m, O.coef_table(m), SK.CLS_LO + 1 - 5, SK.CLS_HI - 1 + 5)
    print(f"m={m}: {nr} m-mers with |R| in 8..25 units, {nrot} with |R(rot)|")
    assert (nr > 0 and nrot > 0) if some else (nr == 0 and nrot == 0)


@pytest.mark.parametrize("k,m", ((63, 21), (47, 19)))
def test_rescan_reads_expire(O, k, m):
    """The reads of the device's re-scan parity cases make the enumerator re-scan: at least once per read on average."""
    reads = SK.rescan_reads(k * 100 + m)
    n = sum(SK.count_expiries(O, r, k, m) for r in reads)
    print(f"k={k} m={m}: {n} expiries in {len(reads)} reads")
    assert n >= len(reads)
    assert any(r[-32:].startswith("A" * 12) for r in reads) and any("C" * 20 in r or "G" * 20 in r or "T" * 20 in r for r in reads)
