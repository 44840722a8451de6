"""The super-k-mer enumerator (Kmers.cpp:509-603) and get_minimizer (Kmers.cpp:367-408) restated in plain Python, with one switch:
full=False is the reference as executed -- the re-scan reads the low 64 bits of the k-mer only (Kmers.cpp:371); full=True removes
that one truncation (brisk_hip_options.minimizer_mode = BRISK_HIP_MINIMIZER_FULL) and nothing else.  The oracle cannot be asked for
full mode, so this file is its yardstick; with full=False it is checked against the oracle k-mer for k-mer (test_minimizer_mode_cpu).
Order keys come from Oracle.key_many and the canonical-form test from the oracle's rcb (the 128-bit "rc" as executed)."""
import os
import random
import sys
from collections import Counter, namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import oracle  # noqa: E402

_CODE = {"A": 0, "C": 1, "T": 2, "G": 3, "a": 0, "c": 1, "t": 2, "g": 3}  # Kmers.cpp:442-444
_ORACLE = None
_KEYS = {}  # (m, canonical m-mer) -> order key
_RC = {}    # (m, m-mer) -> its reverse complement

# kmers: [(lo, hi, minimizer_idx)] as next() yields them; cuts: k-mers per super-k-mer; rets: its minimizer value; by_pos: kmers in read order
Enumerated = namedtuple("Enumerated", "kmers cuts rets by_pos")


def the_oracle():
    global _ORACLE
    if _ORACLE is None:
        oracle.build(ref=False)
        _ORACLE = oracle.Oracle()
    return _ORACLE


def rc_mmer(x, m):
    r = _RC.get((m, x))
    if r is None:
        r, y = 0, x
        for _ in range(m):
            r = (r << 2) | ((y & 3) ^ 2)
            y >>= 2
        _RC[(m, x)] = r
    return r


def keys_of(xs, m):
    missing = sorted({x for x in xs if (m, x) not in _KEYS})
    if missing:
        for x, key in zip(missing, the_oracle().key_many(missing, m)):
            _KEYS[(m, x)] = int(key)
    return [_KEYS[(m, x)] for x in xs]


def canonized(seq, n):  # Kmers.cpp:342-353 as executed
    lo, hi = the_oracle().rcb(seq & (2**64 - 1), seq >> 64, n)
    return seq <= ((hi << 64) | lo)


def get_minimizer(seq, K, m, full):
    """(minimizer value, position, reversed) of the K-mer `seq` (an int of 2K bits)"""
    M = (1 << (2 * m)) - 1
    cur = seq if full else seq & (2**64 - 1)  # the truncation, Kmers.cpp:371
    fwds = [(cur >> (2 * i)) & M for i in range(K - m + 1)]
    cans = [min(f, rc_mmer(f, m)) for f in fwds]
    keys = keys_of(cans, m)
    mini, best, rev, pos = cans[0], keys[0], cans[0] != fwds[0], 0
    for i in range(1, K - m + 1):
        c, h = cans[i], keys[i]
        if h < best:
            pos, mini, rev, best = i, c, c != fwds[i], h
        elif h == best:
            d = K - m - i
            if d < pos:
                pos, mini, rev = d, c, c != fwds[i]
            elif d == pos and not canonized(seq, K):
                pos, mini, rev = d, c, False
    return mini, pos, rev


def enumerate_read(seq, k, m, full):
    """Every k-mer of the read as (kmer_lo, kmer_hi, minimizer_idx), in the order SuperKmerEnumerator::next yields them (a reversed
    vector back to front), the k-mers per super-k-mer (the cuts) and each super-k-mer's returned minimizer value."""
    s = seq.decode() if isinstance(seq, bytes) else seq
    if len(s) < k:
        return Enumerated([], [], [], [])
    KM, MM, w = (1 << (2 * k)) - 1, (1 << (2 * m)) - 1, k - m
    x, mmers = 0, []  # (the keys of the read's own m-mers in one call; what else a re-scan meets is looked up as it comes)
    for i, ch in enumerate(s):
        x = ((x << 2) + _CODE[ch]) & MM
        if i >= m - 1:
            mmers.append(min(x, rc_mmer(x, m)))
    keys_of(mmers, m)
    fwd = rc = cf = cr = 0
    for ch in s[:k - 1]:
        c = _CODE[ch]
        fwd = ((fwd << 2) + c) & (KM >> 2)
        rc = (rc >> 2) + ((c ^ 2) << (2 * (k - 1) - 2))
    rc <<= 2
    for ch in s[k - m - 1:k - 1]:
        c = _CODE[ch]
        cf = ((cf << 2) + c) & (MM >> 2)
        cr = (cr >> 2) + ((c ^ 2) << (2 * m - 2))
    mini, mini_pos, reversed_ = get_minimizer(fwd, k - 1, m, full)
    mini_hash = keys_of([mini], m)[0]
    kmers, cuts, rets, vec, by_pos = [], [], [], [], []
    for p in range(len(s) - k + 1):
        c = _CODE[s[k - 1 + p]]
        fwd = ((fwd << 2) + c) & KM
        rc = (rc >> 2) + ((c ^ 2) << (2 * k - 2))
        cf = ((cf << 2) + c) & MM
        cr = (cr >> 2) + ((c ^ 2) << (2 * m - 2))
        mini_pos = (mini_pos + 1) & 0xFF
        cand = min(cf, cr)
        h = keys_of([cand], m)[0]
        closed, old_rev, ret = False, reversed_, 0
        if mini_pos > w:  # the minimizer left the k-mer
            closed, ret = True, mini
            mini, mini_pos, reversed_ = get_minimizer(fwd, k, m, full)
            mini_hash = keys_of([mini], m)[0]
        elif h < mini_hash:  # a strictly smaller candidate takes over
            closed, ret = True, mini
            mini_hash, mini_pos, mini, reversed_ = h, 0, cand, cand == cr
        km = (rc, w - mini_pos) if reversed_ else (fwd, mini_pos)
        if closed and p > 0:  # a close at p == 0 is ignored
            kmers += vec[::-1] if old_rev else vec
            cuts.append(len(vec))
            rets.append(ret)
            vec = []
        vec.append((km[0] & (2**64 - 1), km[0] >> 64, km[1]))
        by_pos.append(vec[-1])
    if vec:
        kmers += vec[::-1] if reversed_ else vec
        cuts.append(len(vec))
        rets.append(mini)
    return Enumerated(kmers, cuts, rets, by_pos)


def index_of(reads, k, m, full):
    """{(kmer_lo, kmer_hi, minimizer_idx): times inserted} of a bulk count of the reads"""
    idx = Counter()
    for r in reads:
        idx.update(enumerate_read(r, k, m, full).kmers)
    return idx


def revcomp(s):
    return s.translate(str.maketrans("ACGTacgt", "TGCAtgca"))[::-1]


def canonical_kmers(read, k):
    """the canonical k-mers (true reverse complement, as strings) of a read, one per position"""
    out = []
    for p in range(len(read) - k + 1):
        f = read[p:p + k].upper()
        out.append(min(f, revcomp(f)))
    return out


def windows_tie_free(reads, k, m):
    """no window of k - m + 1 consecutive m-mers (a k-mer), nor of k - m (the (k-1)-mer of a read's start), of any read or its reverse
    complement holds two equal canonical m-mers -- the inputs on which get_minimizer's tie rules never run"""
    for r in reads:
        r = r.upper()
        cans = [min(r[i:i + m], revcomp(r[i:i + m])) for i in range(len(r) - m + 1)]
        last = {}
        for i, c in enumerate(cans):
            if c in last and i - last[c] <= k - m:
                return False
            last[c] = i
    return True


def parity_reads():
    """random reads, the periodic and homopolymer reads of the tie tests (test_gpu_parity, test_kmer_query), and the reverse
    complement of every one of them"""
    rng = random.Random(123)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    reads = [rnd(n) for n in (63, 64, 65, 125, 150, 150, 151, 200)]
    for period in (1, 2, 3, 5, 8, 13, 21, 34):
        unit = rnd(period)
        s = (unit * (150 // period + 1))[:150]
        reads.append(s)
        fl = rnd(40)
        reads.append(fl + s[:80] + fl[::-1])
    reads += ["AC" * 100, "ACGTTGCA" * 30, "A" * 70 + "ACGTTGCA" * 10, "T" * 149 + "A", "ACGTTGCATGCA" * 13, "A" * 150, "G" * 97]
    return reads + [revcomp(r) for r in reads]


def tie_free_reads(k, m, n=200, L=150, genome=5000):
    """n reads of L nt, either strand, of a random genome, seeded so that no k-mer window of them holds two equal canonical m-mers"""
    for seed in range(1, 50):
        rng = random.Random(1000 * k + seed)
        g = "".join(rng.choice("ACGT") for _ in range(genome))
        reads = []
        for _ in range(n):
            p = rng.randrange(genome - L + 1)
            r = g[p:p + L]
            reads.append(revcomp(r) if rng.random() < 0.5 else r)
        if windows_tie_free(reads, k, m):
            return reads
    raise AssertionError("no tie-free seed")
