"""Read sets that pin the pair route of k_insert_first (DESIGN.md section 4 finding 22); numpy and the oracle only.

Neighbouring partitions are crafted with the machinery of tests/insert_clean_reads.py (a minimizer made for a chosen partition and
bucket, accepted as the centre of a 105-nt copy of 43 k-mers).  A case is a list of partitions of ONE block of 8192 partitions, so the
touched list of its insert is those partitions in ascending order, whatever the device does (insert_pair_rules.ascending), and what
pairs is known before anything runs.  A partition is built from *heads* -- the read over k-mers [a, a + n) of a centre of its own --
reads *contained* in a head, and *repeats* of a read; its records are its reads, one each.

CASES names them; `case(name)` gives [(partition, [reads])] in ascending order; `expect(name)` what the rule must make of the case
(checked on the CPU by tests/test_insert_pair_cpu.py against insert_pair_rules.walk): per partition "pair", "alone" or "left"."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

import insert_clean_reads as R
from sibling_keys import primed, revcomp

K, M, B = R.K, R.M, R.B
W1 = R.W1
FULL = (0, W1)


def build(cr, part, heads, contained=(), repeats=()):
    """the reads of partition `part`: a fresh centre per head (a, n); contained: (head, a, n), a read inside that head's copy;
    repeats: (read index, times more).  Reads: the heads', then the contained ones in the order given."""
    cs, head_reads, inner, buckets = [], [], {}, set()  # (a bucket per head: no two heads of a partition share routing id and core)
    for h, (a, n) in enumerate(heads):
        mine = [j for j, c in enumerate(contained) if c[0] == h]

        def make():
            c = cr.copies(part, 1)[0]
            return [cr.read(c, a, n, part)] + [cr.read(c, contained[j][1], contained[j][2], part) for j in mine] + [None if cr.one_record(c)[0] in buckets else c], c
        got, c = cr.until(make)
        cs.append(c)
        buckets.add(cr.one_record(c)[0])
        head_reads.append(got[0])
        inner.update(zip(mine, got[1:]))
    reads = head_reads + [inner[j] for j in range(len(contained))]
    for i, times in repeats:
        reads = reads + [reads[i]] * times
    return reads, cs


def cousin(cr, copy, part):
    """the copy with bit 4 of its minimizer's bucket flipped -- the same record words in partition part ^ 1 -- in the orientation in
    which cr.read cuts it as it cuts `copy`, or None"""
    other = primed(cr.O, copy.decode(), K, M, B, 1 << 4)
    if other is None:
        return None
    for r in (other.encode(), revcomp(other).encode()):  # (primed works in the super-k-mer's orientation)
        if cr.one_record(r) == ((cr.one_record(copy)[0]) ^ 16, W1, R.SUFF) and cr.read(r, 0, 30, part ^ 1) is not None:
            return r
    return None


def _parts(cr, count):
    """`count` partition numbers of one block of 8192, ascending; the first is even (its cousin partition is the next number)"""
    block = int(cr.rng.integers(0, 2048))
    offs = sorted(int(x) for x in cr.rng.choice(np.arange(0, 8192, 2), count, replace=False))
    return [block * 8192 + o for o in offs]


# the shapes of the instance-limit cases: heads per partition whose n add up to the size
SHAPES = {1: [(0, 1)], 10: [(0, 10)], 64: [FULL, (0, 21)], 96: [FULL, FULL, (0, 10)], 97: [FULL, FULL, (0, 11)], 128: [FULL, FULL, (0, 42)],
          191: [FULL] * 4 + [(0, 19)], 215: [FULL] * 5}


def _sized(cr, part, size, folds):
    heads = SHAPES[size]
    if not folds or heads[0][1] < 20:
        return build(cr, part, heads)[0]
    # contained and repeated records: the fold decides the size
    return build(cr, part, heads, contained=[(0, 3, 12), (0, 8, 9), (len(heads) - 1, 0, min(5, heads[-1][1]))], repeats=[(0, 2), (len(heads), 1)])[0]


def _limit(cr, sizes, folds=False):
    return [(p, _sized(cr, p, s, folds)) for p, s in zip(_parts(cr, len(sizes)), sizes)]


def _records(cr, counts):
    """partitions of exactly counts[i] records: four heads of 20 k-mers, the rest contained in them: 80 instances each"""
    out = []
    for p, n in zip(_parts(cr, len(counts)), counts):
        contained = [(j % 4, 1 + j // 4, 10) for j in range(n - 4)]
        out.append((p, build(cr, p, [(0, 20)] * 4, contained)[0]))
    return out


def _siblings(cr):
    """A: three centres, contained reads, one read three times; B = A ^ 1: the same strings (cousins: bit 4 of the bucket flipped),
    every read twice"""
    pa = _parts(cr, 1)[0]
    spans, extra = [FULL, (0, 30), (5, 20)], [(0, 4, 15), (1, 10, 12)]
    cs, other = [], []
    for h, (s, n) in enumerate(spans):
        cut = [(s, n)] + [(es, en) for eh, es, en in extra if eh == h]
        for _ in range(2000):
            c = cr.copies(pa, 1)[0]
            o = None if any(cr.one_record(c)[0] == cr.one_record(x)[0] for x in cs) else cousin(cr, c, pa)
            if o is not None and all(cr.read(c, x, y, pa) is not None and cr.read(o, x, y, pa ^ 1) is not None for x, y in cut):
                break
        else:
            raise AssertionError("no cousin copies")
        cs.append(c)
        other.append(o)
    a = [cr.read(c, s, n, pa) for c, (s, n) in zip(cs, spans)] + [cr.read(cs[h], s, n, pa) for h, s, n in extra]
    b = [cr.read(c, s, n, pa ^ 1) for c, (s, n) in zip(other, spans)] + [cr.read(other[h], s, n, pa ^ 1) for h, s, n in extra]
    return [(pa, a + [a[3]] * 2), (pa ^ 1, b + b)]


def _mixed_overlap(cr):
    pa, pb = _parts(cr, 2)
    return [(pa, build(cr, pa, [FULL, (0, 12)])[0]), (pb, build(cr, pb, [(0, 30)], contained=[(0, 13, 30)])[0])]


def _mixed_records(cr):
    pa, pb = _parts(cr, 2)
    hot, _ = build(cr, pb, [FULL, FULL], contained=[(0, 10, 15)], repeats=[(2, 69)])  # 72 records
    return [(pa, build(cr, pa, [FULL])[0]), (pb, hot)]


def _many(cr, count, first_full=False):
    """`count` small eligible partitions: a head of 6 k-mers and a read contained in it; first_full: the first has 64 records"""
    out = []
    for i, p in enumerate(_parts(cr, count)):
        if i == 0 and first_full:
            out.append((p, build(cr, p, [(0, 20)] * 4, [(j % 4, 1 + (j // 4) % 8, 5 + (j // 4) // 8) for j in range(60)])[0]))
        else:
            out.append((p, build(cr, p, [(0, 6)], contained=[(0, 2, 3)])[0]))
    return out


CASES = {
    # name: (builder, what the rule makes of the partitions in ascending order)
    "rec-32-32": (lambda cr: _records(cr, (32, 32)), ("pair", "pair")),
    "rec-32-33": (lambda cr: _records(cr, (32, 33)), ("alone", "alone")),
    "inst-96-96": (lambda cr: _limit(cr, (96, 96)), ("pair", "pair")),
    "inst-1-191": (lambda cr: _limit(cr, (1, 191)), ("pair", "pair")),
    "inst-128-64": (lambda cr: _limit(cr, (128, 64)), ("pair", "pair")),
    "inst-96-97": (lambda cr: _limit(cr, (96, 97, 10)), ("alone", "pair", "pair")),  # A alone, B heads the next pair
    "fold-96-96": (lambda cr: _limit(cr, (96, 96), True), ("pair", "pair")),
    "fold-1-191": (lambda cr: _limit(cr, (1, 191), True), ("pair", "pair")),
    "fold-128-64": (lambda cr: _limit(cr, (128, 64), True), ("pair", "pair")),
    "fold-96-97": (lambda cr: _limit(cr, (96, 97, 10), True), ("alone", "pair", "pair")),
    "siblings": (_siblings, ("pair", "pair")),
    "mixed-overlap": (_mixed_overlap, ("alone", "alone")),     # B by the table path
    "mixed-records": (_mixed_records, ("alone", "left")),      # B: more than 64 records
    "mixed-big-a": (lambda cr: _limit(cr, (215, 10)), ("left", "alone")),  # A's own instances exceed 192
    "batch-3": (lambda cr: _many(cr, 3), ("pair", "pair", "alone")),
    "batch-65": (lambda cr: _many(cr, 65), ("pair",) * 64 + ("alone",)),
    "batch-66-shifted": (lambda cr: _many(cr, 66, True), ("alone",) + ("pair",) * 62 + ("alone", "pair", "pair")),  # lanes 63 | 64: no pair across
    "single": (lambda cr: _many(cr, 1), ("alone",)),
}
SAT_CASES = ("fold-96-96", "siblings", "batch-3")  # also into a saturating index (the SAT instantiation)

_built = {}


def _build_all():
    if _built:
        return
    cr = R.Crafter(2207)
    try:
        for name, (make, _) in CASES.items():
            _built[name] = make(cr)
    finally:
        cr.close()


def case(name):
    _build_all()
    return _built[name]


def expect(name):
    return CASES[name][1]


def pack(parts, seed=0):
    """(flat, offsets) of a case's reads, shuffled"""
    reads = [r for _, rs in parts for r in rs]
    rng = np.random.default_rng([seed, 0xab])
    return R._pack([reads[i] for i in rng.permutation(len(reads))])


def partitions_of(O, reads):
    """{partition: records in arrival order} of (flat, offsets) (fold_group_rules.partitions_of)"""
    import fold_group_rules as G
    return G.partitions_of(O, reads, 4)
