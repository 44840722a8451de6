"""Read sets that pin k_insert_first's table-free path (DESIGN.md section 4 finding 19); numpy and the oracle only.

Geometry: k63 m21 b14 at the default 2^24 partitions: a partition is 16 buckets, w = k - m = 42, suff_reduc = 4, so idx' runs over
[4, 46], the common frame ends at E = 47 and every k-mer window covers the frame's nucleotides [k - m, k - b) = [42, 49): the *core*,
the 14 bits of the minimizer's hash that are neither in the 28-bit bucket nor cut out with it.

A partition is *table-free* when the containment fold proves that no two of its k-mer instances are equal: no two records that
survive the fold have the same routing id, intersecting idx' ranges and the same core, and the fold took at most 16 heads.

Partitions are crafted, not searched for: the minimizer hash is invertible (the oracle's mix_inv), so a minimizer is made for a
chosen 42-bit hash -- [6 bits | bucket: 28 | 8 bits] -- and accepted as the *centre* of a 105-nt *copy* (random 42-nt flanks) when
the oracle cuts the copy into one super-k-mer of 43 k-mers in the chosen bucket.  Any number of centres share one partition, and
two share one bucket with different remaining bits.  A read over k-mers [a, a + n) of a copy is `copy[a : a + 62 + n]`.

The kinds of partition:
  once-S      S in 64, 65, 128, 129, 192: full copies of different centres and one partial, every k-mer once: S instances, clean
  folds-S     the same with a contained 15-k-mer read twice more and one full copy read again: S instances after the fold, clean
  loci        two centres of one bucket, both whole: their ranges intersect, their cores differ: clean
  overlap     one copy read as k-mers [0, 30) and [13, 43), never whole: 17 k-mers count 2: not clean
  chain       one copy as [0, 16), [8, 24), [16, 32): not clean
  both-sides  one copy as [6, 30), [0, 12), [14, 34): the first read is overlapped from both sides: not clean
  subst       a copy and the same copy with one nucleotide of the right flank changed: same bucket, range and core, the k-mers over
              the change differ and the others count 2: not clean
  heads       4 k-mers each of 18 centres: all distinct, but more heads than the fold takes (WI_FOLD_TRIPS = 16): not clean
  hot         two whole copies and a 15-k-mer read of one of them 300 times: more than 64 records, left over to k_insert

`census(O, reads)` runs the fold's rules over the oracle's records of every read (their exchange format: string, bucket, n, idx0')
and counts per set the partitions, those k_insert_first takes (LEAN: at most 64 records, at most 192 instances after the fold),
those of them that are certainly table-free (CLEAN) and those that may go either way (AMBIG: none; the outcome does not depend on
the order the records arrive in, see `_partition_state`)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

import insert_lean3_reads as R3
from density_reads import _offsets

K, M, B = 63, 21, 14
W1 = K - M + 1        # k-mers of a full super-k-mer
KB = K - B            # nucleotides of a compacted k-mer
SUFF = (M - B + 1) // 2   # suff_reduc
E = SUFF + K - M + 1  # the common frame's end: every record's idx0' + n is at most E
CORE_NT = (K - M, K - B)  # the frame's nucleotides every k-mer window covers
CORE = ((1 << (2 * CORE_NT[1])) - 1) ^ ((1 << (2 * CORE_NT[0])) - 1)
FOLD_TRIPS = 16
SIZES = (64, 65, 128, 129, 192)
_ENC = "ACTG"  # the oracle's 2-bit code, first nucleotide in the top bits


def _decode(x, n):
    return "".join(_ENC[(x >> (2 * (n - 1 - i))) & 3] for i in range(n)).encode()


def sub(copy, a, n):
    """the read over k-mers [a, a + n) of a copy"""
    return copy[a:a + K - 1 + n]


class Crafter:
    def __init__(self, seed):
        import oracle

        self.O = oracle.Oracle()
        self.rng = np.random.default_rng([seed, 0xc1ea])
        self.h = self.O.index_new(K, M, B)  # (for O.records: nothing is inserted)
        self.parts = set()

    def close(self):
        self.O.index_free(self.h)

    def partition(self):
        while True:
            p = int(self.rng.integers(0, 1 << 24))
            if p not in self.parts:
                self.parts.add(p)
                return p

    def one_record(self, read):
        c, bucket, n, idx0 = self.O.records(self.h, read, K, M, B)
        return (int(bucket[0]), int(n[0]), int(idx0[0])) if len(n) == 1 else None

    def copies(self, part, count, bucket=None):
        """`count` copies of different centres in partition `part` (all in `bucket` if given)"""
        O, rng, out, used = self.O, self.rng, [], set()
        while len(out) < count:
            bk = bucket if bucket is not None else part * 16 + int(rng.integers(0, 16))
            hsh = (int(rng.integers(0, 2)) << 36) | (bk << 8) | int(rng.integers(0, 256))  # a small hash: few m-mers order before it
            if hsh in used:
                continue
            used.add(hsh)
            x = int(O.mix_inv_many([hsh], M)[0])
            if int(O.class_many([x], M)[0]) != 0:
                continue
            copy = R3._copy(O, rng, _decode(x, M))
            if copy is None or self.one_record(copy) != (bk, W1, SUFF):
                continue
            out.append(copy)
        return out

    def read(self, copy, a, n, part):
        """the read over k-mers [a, a + n) of a copy, or None where the oracle does not make it one record of the copy's partition
        (a read that begins inside the copy may be given another minimizer there than the whole copy is)"""
        r = sub(copy, a, n)
        got = self.one_record(r)
        return r if got is not None and got[0] >> 4 == part and got[1:] == (n, SUFF + a) else None

    def until(self, make):
        """make() until none of the reads it returns is None"""
        for _ in range(200):
            got = make()
            if all(r is not None for r in got[0]):
                return got
        raise AssertionError("no copy takes these reads")


def _once(cr, size, folds=False):
    part = cr.partition()
    full, rest = divmod(size, W1)

    def make():
        cs = cr.copies(part, full + (1 if rest else 0))
        reads = cs[:full] + ([cr.read(cs[full], 0, rest, part)] if rest else [])
        if folds:
            reads += [cr.read(cs[0], int(cr.rng.integers(0, 15)), 15, part)] * 2 + [cs[0]]
        return reads, cs
    return cr.until(make)[0]


def _folds(cr, size):
    return _once(cr, size, folds=True)


def _loci(cr):
    part = cr.partition()
    return cr.copies(part, 2, bucket=part * 16 + int(cr.rng.integers(0, 16)))


def _spans(cr, spans):
    part = cr.partition()

    def make():
        c = cr.copies(part, 1)[0]
        return [cr.read(c, a, n, part) for a, n in spans], c
    return cr.until(make)[0]


def _subst(cr):
    part = cr.partition()
    c = cr.copies(part, 1)[0]
    want = cr.one_record(c)
    for pos in cr.rng.permutation(np.arange(K + 8, 2 * K - M - 4)):  # in the right flank: k-mers [pos - 62, 43) lie over it
        for ch in b"ACGT":
            if ch != c[pos]:
                v = c[:pos] + bytes([ch]) + c[pos + 1:]
                if cr.one_record(v) == want:
                    return [c, v]
    raise AssertionError("no substitution keeps the copy one super-k-mer")


def _heads(cr):
    part = cr.partition()
    reads = []
    while len(reads) < FOLD_TRIPS + 2:
        r = cr.read(cr.copies(part, 1)[0], 0, 4, part)
        if r is not None and r not in reads:
            reads.append(r)
    return reads


def _hot(cr):
    part = cr.partition()

    def make():
        cs = cr.copies(part, 2)
        return [cr.read(cs[0], 10, 15, part)], cs
    reads, cs = cr.until(make)
    return cs, reads[0]


def _pack(reads):
    flat = np.frombuffer(b"".join(reads), np.uint8).copy()
    return flat, _offsets(np.array([len(r) for r in reads], np.int64))


def _shuffled(cr, groups):
    reads = [r for g in groups for r in g]
    return _pack([reads[i] for i in cr.rng.permutation(len(reads))])


_sets = {}


def _build():
    if _sets:
        return
    cr = Crafter(181)
    try:
        _sets["once"] = _shuffled(cr, [_once(cr, s) for s in SIZES for _ in range(6)])
        _sets["folds"] = _shuffled(cr, [_folds(cr, s) for s in SIZES for _ in range(6)])
        _sets["loci"] = _shuffled(cr, [_loci(cr) for _ in range(14)])
        table = ([_spans(cr, [(0, 30), (13, 30)]) for _ in range(8)] + [_spans(cr, [(0, 16), (8, 16), (16, 16)]) for _ in range(4)]
                 + [_spans(cr, [(6, 24), (0, 12), (14, 20)]) for _ in range(4)] + [_subst(cr) for _ in range(8)] + [_heads(cr) for _ in range(4)])
        _sets["table"] = _shuffled(cr, table)
        _sets["mixed"] = _shuffled(cr, table[::2] + [_once(cr, 64) for _ in range(10)] + [_folds(cr, 129) for _ in range(10)])
        cs, hot = _hot(cr)
        calm = [_once(cr, 65) for _ in range(12)]
        _sets["hot"] = (calm, cs, hot)
    finally:
        cr.close()


SETS = ("once", "folds", "loci", "table", "mixed")


def get(name):
    """(flat, offsets) of a set"""
    _build()
    return _sets[name]


def hot():
    """(reads of 12 clean partitions, the two whole copies of the hot partition, its 15-k-mer read)"""
    _build()
    return _sets["hot"]


def hot_reads(times):
    calm, cs, h = hot()
    flat = [r for g in calm for r in g]
    return flat[:6] + cs + [h] * times + flat[6:]


def _partition_state(recs):
    """The fold's outcome for one partition's records [(bucket, idx0', n, C)].  Heads are taken by decreasing n, so a head is
    maximal and every record it contains closes with it: the survivors are the maximal records (identical ones once), one round
    each, whatever the order of arrival.  A record B still open in the round of head A that meets A (bucket, range, core) is either
    a survivor -- then the pair of survivors meets -- or contained in a survivor C, whose range holds B's and whose bucket and core
    are B's -- then C meets A.  So "not clean" is: two survivors meet, or there are more survivors than rounds."""
    fr = set()
    for bucket, i0, n, c in recs:
        end = i0 + n
        assert SUFF <= i0 and end <= E
        lo = 2 * (E - end)
        fr.add((bucket, i0, end, c << lo, ((1 << (2 * (n + KB - 1))) - 1) << lo))
    fr = sorted(fr)
    inside = lambda b, a: b[0] == a[0] and a[1] <= b[1] and b[2] <= a[2] and (a[3] & b[4]) == b[3]
    top = [b for b in fr if not any(a is not b and inside(b, a) for a in fr)]
    meet = any(a[0] == b[0] and a[1] < b[2] and b[1] < a[2] and ((a[3] ^ b[3]) & CORE) == 0 for i, a in enumerate(top) for b in top[i + 1:])
    inst = sum(t[2] - t[1] for t in top)
    lean = len(recs) <= 64 and inst <= 192
    return {"records": len(recs), "survivors": len(top), "instances": inst, "lean": lean, "clean": lean and not meet and len(top) <= FOLD_TRIPS}


def census(O, reads):
    """per-partition states of a read set, and the counts the GPU test asserts"""
    flat, offs = reads
    raw, o = flat.tobytes(), offs.astype(np.int64)
    h = O.index_new(K, M, B)
    parts = {}
    try:
        for i in range(len(o) - 1):
            c, bucket, n, idx0 = O.records(h, raw[o[i]:o[i + 1]], K, M, B)
            for j in range(len(n)):
                big = sum(int(w) << (64 * t) for t, w in enumerate(c[j]))
                parts.setdefault(int(bucket[j]) >> 4, []).append((int(bucket[j]), int(idx0[j]), int(n[j]), big))
    finally:
        O.index_free(h)
    states = {p: _partition_state(r) for p, r in parts.items()}
    return {"partitions": len(states), "LEAN": sum(s["lean"] for s in states.values()), "CLEAN": sum(s["clean"] for s in states.values()), "AMBIG": 0,
            "sizes": sorted(s["instances"] for s in states.values() if s["clean"]), "states": states}
