"""Read sets that pin k_insert_first's third instance slot (DESIGN.md section 4 finding 16) at its edges; numpy and the oracle only.

Geometry: k63 m21 b14 at the default 2^24 partitions, so a partition is one minimizer's 16 buckets and w = k - m = 42.

A *copy* of a locus is 105 nt: a 21-nt centre between two random 42-nt flanks, accepted when the oracle cuts it into one
super-k-mer of w + 1 = 43 k-mers (the centre is the minimizer of every one of them; reads of the loci are given on that
strand only: the acceptance says nothing about the other).  D copies of one centre with flanks of
their own put 43 D distinct k-mers into one partition, a read over the first 62 + n nt of a further copy adds n < 43 more, and
since every k-mer is covered once and no record contains another, the partition holds exactly as many k-mer instances after the
containment fold as distinct k-mers.  CLASSES lists the sizes built that way: on both sides of the second slot's end (128 | 129)
and of the third's (191, 192 | 193).  Some partitions of more than 64 records (sub-ranges of one copy: few k-mers, many
records) and low-coverage background reads of a random genome come with them.

`set_one()` is that.  `set_two()` has the same kinds of partition with, on chosen loci, a sub-range of 15 k-mers of one copy
read another two or three times (coverage 3 to 4 there): contained records the fold has to close.  Where the sum of counts
stays within 192 the partition must still go lean; on some 191- and 192-k-mer loci it does not, and whether those go lean
depends on what the fold closes (AMBIG in `census`).

`census(O, reads)` gives the oracle's per-partition numbers: distinct k-mers, the sum of counts (= the instances before the
fold, an upper bound of those after it) and records, and from them the sets the tests work with."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

from density_reads import _LETTERS, _offsets, concat_reads, dense_reads

K, M, B = 63, 21, 14
W1 = K - M + 1  # k-mers of a full super-k-mer
COPY = 2 * K - M  # nt of a copy
SLOT = 64
CLASSES = (128, 129, 191, 192, 193)


def _letters(rng, n):
    return _LETTERS[rng.integers(0, 4, n, dtype=np.uint8)].tobytes()


def _one_full_superkmer(O, seq):
    n = O.enumerate(seq, K, M)[1]
    return len(n) == 1 and int(n[0]) == W1


def _centres(O, rng, want):
    """centres of full super-k-mers of a random sequence that stand as copies of their own and take new flanks readily"""
    g = _letters(rng, 400000)
    n = O.enumerate(g, K, M)[1].astype(np.int64)
    first = np.cumsum(n) - n
    out, seen = [], set()
    for p in first[n == W1]:
        c = g[p + W1 - 1:p + W1 - 1 + M]
        if c in seen or not _one_full_superkmer(O, g[p:p + COPY]):
            continue
        seen.add(c)
        out.append(c)
        if len(out) == want:
            return out
    raise AssertionError("too few full super-k-mers in the random sequence")


def _copy(O, rng, centre):
    for _ in range(400):
        f = _letters(rng, 2 * (W1 - 1))
        c = f[:W1 - 1] + centre + f[W1 - 1:]
        if _one_full_superkmer(O, c):
            return c
    return None


def _locus_reads(O, rng, centre, distinct):
    """reads that put exactly `distinct` k-mers of one minimizer into its partition, each k-mer once"""
    full, part = divmod(distinct, W1)
    copies = [_copy(O, rng, centre) for _ in range(full + (1 if part else 0))]
    if any(c is None for c in copies):
        return None, None
    reads = copies[:full] + ([copies[full][:K - 1 + part]] if part else [])
    return reads, copies


def _sub_reads(O, h, copy, spans, want):
    """the first `want` reads over k-mers [a, a + n) of `copy`, (a, n) from `spans`, that are one record of the copy's partition
    (a read that begins inside the copy may be given another minimizer there than the whole copy is)"""
    home = int(O.records(h, copy, K, M, B)[1][0])
    out = []
    for a, n in spans:
        r = copy[a:a + K - 1 + n]
        bucket, nk = O.records(h, r, K, M, B)[1:3]
        if len(bucket) == 1 and int(bucket[0]) >> 4 == home >> 4 and int(nk[0]) == n:
            out.append(r)
            if len(out) == want:
                break
    return out


def _pack(reads):
    flat = np.frombuffer(b"".join(reads), np.uint8).copy()
    return flat, _offsets(np.array([len(r) for r in reads], np.int64))


def _build(seed, per_class, extra):
    """per_class: {distinct: loci}; extra: {distinct: loci that get a 15-k-mer sub-range read 2 or 3 more times}"""
    import oracle

    O = oracle.Oracle()
    rng = np.random.default_rng([seed, 0x1ea3])
    h = O.index_new(K, M, B)  # (for O.records: nothing is inserted)
    n_many = 6
    centres = _centres(O, rng, sum(per_class.values()) + n_many + 40)
    reads, hot, at = [], None, 0
    for distinct in CLASSES:
        done = 0
        while done < per_class[distinct]:
            centre = centres[at]
            at += 1
            rs, copies = _locus_reads(O, rng, centre, distinct)
            if rs is None:  # (a centre that takes few flanks: the next one)
                continue
            if done < extra.get(distinct, 0):
                sub = _sub_reads(O, h, copies[0], [(int(a), 15) for a in rng.permutation(W1 - 15)], 1)
                rs = rs + sub * (2 + done % 2)
            if distinct == 192 and hot is None:
                hot = (rs, copies[0])
            reads += rs
            done += 1
    for _ in range(n_many):  # more than 64 records, few k-mers: 66 distinct sub-ranges of one copy
        sub = []
        while len(sub) < 66:
            c = _copy(O, rng, centres[at])
            at += 1
            sub = _sub_reads(O, h, c, [(a, n) for a in range(0, 18) for n in range(20, 26)], 66) if c is not None else []
        reads += sub
    O.index_free(h)
    order = rng.permutation(len(reads))
    special = _pack([reads[i] for i in order])
    background = dense_reads(1500, K, 1000000, seed, e=0.0, p_n=0.0, n_special=0, lower_share=0.0, ragged_share=0.01)
    return concat_reads([background, special]), hot


_sets = {}


def set_one():
    """every k-mer of the loci once"""
    if 1 not in _sets:
        _sets[1] = _build(171, {128: 24, 129: 30, 191: 24, 192: 30, 193: 24}, {})
    return _sets[1][0]


def hot_locus():
    """(the reads of one 192-k-mer locus of set_one, one full copy of it)"""
    set_one()
    return _sets[1][1]


def set_two():
    """other loci; coverage 3 to 4 on a sub-range of all 128-, 129- and 193-k-mer loci and of 8 each of the 191- and 192-k-mer ones"""
    if 2 not in _sets:
        _sets[2] = _build(172, {128: 24, 129: 40, 191: 24, 192: 24, 193: 24}, {128: 24, 129: 40, 191: 8, 192: 8, 193: 24})
    return _sets[2][0]


def census(O, reads):
    """The oracle's index of `reads` per partition (bucket id >> 4): {"distinct", "sum", "records"} as dicts over all partitions,
    and the partition sets S3 (need the third slot and must go lean), OVER (must be left over), AMBIG (either), per CLASSES the
    partitions of exactly that many distinct k-mers and as many instances."""
    flat, offs = reads
    h = O.index_new(K, M, B)
    try:
        O.index_insert_reads(h, flat, offs)
        lo, hi, idx, cnt = O.index_dump(h)
        part = O.bucket_ids(h, lo, hi, idx) >> 4
        u, inv = np.unique(part, return_inverse=True)
        distinct = np.bincount(inv, minlength=len(u))
        total = np.bincount(inv, weights=cnt.astype(np.float64), minlength=len(u)).astype(np.int64)
        assert int(cnt.max()) < 200  # (the oracle's counts wrap at 256: these are exact)
        raw, o = flat.tobytes(), offs.astype(np.int64)
        rec = np.concatenate([O.records(h, raw[o[i]:o[i + 1]], K, M, B)[1] >> 4 for i in range(len(o) - 1) if o[i + 1] - o[i] >= K])
    finally:
        O.index_free(h)
    ru, rc = np.unique(rec, return_counts=True)
    assert np.array_equal(ru, u)
    s3 = (distinct > 2 * SLOT) & (total <= 3 * SLOT) & (rc <= 64)
    over = (distinct > 3 * SLOT) | (rc > 64)
    ambig = (distinct <= 3 * SLOT) & (total > 3 * SLOT) & (rc <= 64)
    return {"partitions": int(len(u)), "S3": int(s3.sum()), "OVER": int(over.sum()), "AMBIG": int(ambig.sum()), "many_records": int((rc > 64).sum()),
            "exact": {c: int(((distinct == c) & (total == c)).sum()) for c in CLASSES},
            "at": {c: int((distinct == c).sum()) for c in CLASSES},
            "folding": int(((total > distinct) & (distinct > 2 * SLOT) & (rc <= 64)).sum())}
