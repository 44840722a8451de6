"""Inputs shared by test_scan_keys_cpu.py (no device) and test_scan_keys.py (device): the m-mers the order-key comparison runs on, the
reads of the re-scan parity cases, and numpy restatements of the decycling sums and of the enumerator's expiries.  Nothing here
touches a device."""
import random

import numpy as np

import oracle

EPS = 1e-6
CODE = {"A": 0, "C": 1, "T": 2, "G": 3}  # Kmers.cpp:442-444


def mmer(s: str) -> int:
    v = 0
    for c in s:
        v = (v << 2) | CODE[c]
    return v


def fold_sums(xs: np.ndarray, m: int, coef: np.ndarray):
    """R(x) and R(rot(x)) of Decycling.cpp:17-24,41 for an array of m-mers: R = sum_{i=0}^{m-2} coef[4(m-1-i) + nt_i],
    R(rot) = sum_{i=1}^{m-1} coef[4(m-i) + nt_i], nt_i = nucleotide i counted from the low end.  (numpy adds in another order than
    the reference: 1e-15 apart, nothing next to the 6e-8 unit the tables are rounded to.)"""
    xs = np.asarray(xs, np.uint64)
    r = np.zeros(len(xs))
    rr = np.zeros(len(xs))
    for i in range(m):
        nt = ((xs >> np.uint64(2 * i)) & np.uint64(3)).astype(np.int64)
        if i + 1 < m:
            r += coef[4 * (m - 1 - i) + nt]
        if i >= 1:
            rr += coef[4 * (m - i) + nt]
    return r, rr


# ---- the chunk tables and the integer class decode, restated (brisk_scan.hip: cls_nch .. decy_class_guarded; brisk_hip_create) ----
CLS_W, CLS_LO, CLS_HI, CLS_BIAS = 5, 12, 21, 1 << 31


def chunk_layout(m: int):
    """[(first nt, nts)] of the chunks of an m-mer, low nts first"""
    n = (m + CLS_W - 1) // CLS_W
    out, off = [], 0
    for c in range(n):
        wd = m // n + (1 if c < m % n else 0)
        out.append((off, wd))
        off += wd
    return out


def table_sums(xs: np.ndarray, m: int, coef: np.ndarray):
    """The integer sums A, B (units of 2^-24) the device adds up from its chunk tables: every chunk's share of R and of R(rot) is
    added up in the host builder's order and rounded to a unit on its own."""
    xs = np.asarray(xs, np.uint64)
    A = np.zeros(len(xs), np.int64)
    B = np.zeros(len(xs), np.int64)
    rnd = lambda v: np.where(v >= 0, np.floor(v + 0.5), -np.floor(-v + 0.5)).astype(np.int64)  # llround
    for off, wd in chunk_layout(m):
        a = np.zeros(len(xs))
        b = np.zeros(len(xs))
        for i in range(off, off + wd):
            nt = ((xs >> np.uint64(2 * i)) & np.uint64(3)).astype(np.int64)
            if i + 1 < m:
                a = a + coef[4 * (m - 1 - i) + nt]
            if i >= 1:
                b = b + coef[4 * (m - i) + nt]
        A += rnd(np.ldexp(a, 24))
        B += rnd(np.ldexp(b, 24))
    return A, B


def decode_plain(a: np.ndarray, b: np.ndarray):
    """(class or 2, guard) from the signed sums by the plain comparisons: a sum certainly above eps is >= CLS_HI, certainly below
    <= CLS_LO, anything between (either sign, either sum) is the guard band."""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    guard = ((np.abs(a) > CLS_LO) & (np.abs(a) < CLS_HI)) | ((np.abs(b) > CLS_LO) & (np.abs(b) < CLS_HI))
    c0 = (a >= CLS_HI) & (b <= CLS_LO)
    c1 = (a <= -CLS_HI) & (b >= -CLS_LO)
    return np.where(c0, 0, np.where(c1, 1, 2)), guard


def decode_biased(a: np.ndarray, b: np.ndarray):
    """The same from the 64-bit word the device holds: the sum of signed words a_c + b_c * 2^32 whose chunk-0 entry carries 2^31 in
    both halves; low and high word taken apart without a borrow fix, |.| - (CLS_LO + 1) as a wrapping sum of absolute differences
    (v_sad_u32) against the bias, one unsigned minimum and compare for the band, unsigned compares for the classes."""
    u64, u32m = np.uint64, np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        word = np.asarray(a, np.int64).astype(u64) + (np.asarray(b, np.int64).astype(u64) << u64(32)) + u64((CLS_BIAS << 32) + CLS_BIAS)
    lo, hi = (word & u32m).astype(np.int64), (word >> u64(32)).astype(np.int64)
    sad = lambda v: (np.abs(v - CLS_BIAS) - (CLS_LO + 1)) & 0xFFFFFFFF
    guard = np.minimum(sad(lo), sad(hi)) <= CLS_HI - CLS_LO - 2
    c0 = (lo >= CLS_BIAS + CLS_HI) & (hi <= CLS_BIAS + CLS_LO)
    c1 = (lo <= CLS_BIAS - CLS_HI) & (hi >= CLS_BIAS - CLS_LO)
    return np.where(c0, 0, np.where(c1, 1, 2)), guard


def periodic_mmers(m: int):
    """every m-mer of period 1, 2 or 3 (all units, so all rotations)"""
    out = set()
    for p in (1, 2, 3):
        for u in range(4 ** p):
            unit = "".join("ACTG"[(u >> (2 * j)) & 3] for j in range(p))
            out.add(mmer((unit * m)[:m]))
    return sorted(out)


def padded_mmers(m: int, rng: random.Random, per_j: int = 8):
    """A^j . s, j = 1..m-1: what a zero-padded window of the k > 32 re-scan looks like"""
    return [rng.getrandbits(2 * (m - j)) for j in range(1, m) for _ in range(per_j)]


def near_eps_mmers(m: int, coef: np.ndarray, seed: int, n_sample: int = 1 << 20, take: int = 128):
    """From a seeded sample: the m-mers whose R(x), and those whose R(rot x), lie nearest to +eps and to -eps (`take` each)."""
    rs = np.random.RandomState(seed)
    xs = (rs.randint(0, 1 << 31, n_sample).astype(np.uint64) << np.uint64(31) | rs.randint(0, 1 << 31, n_sample).astype(np.uint64)) & np.uint64((1 << (2 * m)) - 1)
    r, rr = fold_sums(xs, m, coef)
    out = []
    for v in (r, rr):
        for e in (EPS, -EPS):
            out.append(xs[np.argsort(np.abs(v - e), kind="stable")[:take]])
    return np.concatenate(out)


def band_mmers(m: int, coef: np.ndarray, seed: int, want: int = 64, lo_units: float = 14.0, hi_units: float = 19.0):
    """m-mers whose R(x) certainly lies inside the guard band around +-eps: between lo_units and hi_units of 2^-24 in size, one unit
    inside the band's edges, the room the tables' rounding can take.  A random sample practically never holds one, so they are put
    together: R is a sum over nucleotides, R(hi | lo) = R(hi | 0) + R(lo) - R(0); to seeded upper parts the lower part (10 nucleotides
    at most) that brings the sum into the band is looked up among the sorted sums of all lower parts.  Fewer than `want`, or none,
    where the m-mers are too few to hold any (m = 11)."""
    rs = np.random.RandomState(seed)
    nl = min(m // 2, 10)
    lows = np.arange(4 ** nl, dtype=np.uint64)
    r0 = fold_sums(np.zeros(1, np.uint64), m, coef)[0][0]
    rl = fold_sums(lows, m, coef)[0] - r0
    order = np.argsort(rl, kind="stable")
    srt = rl[order]
    unit = 2.0 ** -24
    n_hi = min(1 << 16, 4 ** (m - nl))
    if n_hi == 4 ** (m - nl):
        his = np.arange(n_hi, dtype=np.uint64)
    else:
        his = (rs.randint(0, 1 << 31, n_hi).astype(np.uint64) << np.uint64(31) | rs.randint(0, 1 << 31, n_hi).astype(np.uint64)) & np.uint64((1 << (2 * (m - nl))) - 1)
    his = his << np.uint64(2 * nl)
    rh = fold_sums(his, m, coef)[0]
    out = []
    for sign in (1.0, -1.0):
        a, b = sorted((sign * lo_units * unit, sign * hi_units * unit))
        i = np.searchsorted(srt, a - rh, side="left")
        ok = (i < len(srt)) & (srt[np.minimum(i, len(srt) - 1)] <= b - rh)
        out.append(his[ok] | lows[order[i[ok]]])
    out = np.unique(np.concatenate(out))
    rs.shuffle(out)
    return out[:want]


def count_band_mmers(m: int, coef: np.ndarray, lo_units: float, hi_units: float):
    """How many of ALL 4^m m-mers have |R(x)|, and how many |R(rot x)|, between lo_units and hi_units of 2^-24: R is a sum over
    nucleotides, so every m-mer's sum is an upper part's share plus a lower part's; the lower parts' shares sorted, two binary
    searches per upper part count the pairs inside the interval."""
    def shares(which, first, last):  # the sums' shares of nucleotides [first, last), indexed by their value (low nucleotide first)
        arr = np.zeros(1)
        for i in range(first, last):
            if which == 0:
                s = coef[4 * (m - 1 - i):4 * (m - 1 - i) + 4] if i + 1 < m else np.zeros(4)
            else:
                s = coef[4 * (m - i):4 * (m - i) + 4] if i >= 1 else np.zeros(4)
            arr = (s[:, None] + arr[None, :]).ravel()
        return arr

    nl = (m + 1) // 2
    unit = 2.0 ** -24
    out = []
    for which in (0, 1):
        srt, hi = np.sort(shares(which, 0, nl)), shares(which, nl, m)
        n = 0
        for sign in (1.0, -1.0):
            a, b = sorted((sign * lo_units * unit, sign * hi_units * unit))
            n += int((np.searchsorted(srt, b - hi, side="right") - np.searchsorted(srt, a - hi, side="left")).sum())
        out.append(n)
    return tuple(out)


# ---- reads of the re-scan parity cases --------------------------------------------------------------------------------------------
def rescan_reads(seed: int, n: int = 256, L: int = 150):
    """n reads of L bp: ordinary seeded ones, homopolymer runs, period-2 and period-3 stretches, and reads in which the last 32
    nucleotides of many k-mers -- those of the read itself among them -- begin with 12 or more A (zero-padded windows that tie with
    each other and with the all-A m-mer)."""
    rng = random.Random(seed)
    rnd = lambda k: "".join(rng.choice("ACGT") for _ in range(k))
    reads = []
    while len(reads) < n:
        kind = len(reads) % 4
        if kind == 0:
            s = rnd(L)
        elif kind == 1:  # a homopolymer run somewhere
            run = rng.choice("ACGT") * rng.randint(20, 110)
            at = rng.randint(0, L - len(run))
            s = rnd(at) + run + rnd(L - at - len(run))
        elif kind == 2:  # a period-2 or period-3 stretch
            unit = rnd(rng.choice((2, 3)))
            st = (unit * L)[: rng.randint(30, 120)]
            at = rng.randint(0, L - len(st))
            s = rnd(at) + st + rnd(L - at - len(st))
        else:  # the last 32 nucleotides begin with 12 or more A; further A runs upstream
            na = rng.randint(12, 32)
            tail = "A" * na + rnd(32 - na)
            body = rnd(L - 32)
            at = rng.randint(0, L - 32 - 24)
            body = body[:at] + "A" * rng.randint(12, 24) + body[at:]
            s = body[: L - 32] + tail
        assert len(s) == L
        reads.append(s)
    return reads


def count_expiries(O, read: str, k: int, m: int) -> int:
    """The enumerator's state machine (Kmers.cpp:509-603) from the oracle's own pieces: how often the minimizer leaves the k-mer and
    get_minimizer re-scans (the close at step 0 included, as the scan pays for it too)."""
    w = k - m
    nk = len(read) - k + 1
    if nk <= 0:
        return 0
    M = (1 << (2 * m)) - 1
    code = [CODE[c] for c in read]
    fw = []
    x = 0
    for i, c in enumerate(code):
        x = ((x << 2) | c) & M
        if i >= m - 1:
            fw.append(x)
    cands = [min(f, O.rcbc(f, m)) for f in fw]  # cands[j]: the canonical m-mer ending at nucleotide j + m - 1
    keys = O.key_many(cands, m)

    def kmer(p, K):
        return oracle.str2kmer(read[p:p + K])

    mini, pos, _ = O.get_minimizer(*kmer(0, k - 1), k - 1, m)
    mini_hash = int(O.key_many([mini], m)[0])
    n_exp = 0
    for p in range(nk):
        h = int(keys[k - 1 + p - (m - 1)])
        pos += 1
        if pos > w:
            n_exp += 1
            mini, pos, _ = O.get_minimizer(*kmer(p, k), k, m)
            mini_hash = int(O.key_many([mini], m)[0])
        elif h < mini_hash:
            mini_hash, pos = h, 0
    return n_exp
