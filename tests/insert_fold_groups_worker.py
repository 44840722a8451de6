"""Read sets and worker of tests/test_insert_fold_groups.py: crafted partitions at k63 m21 b14 for the grouped fold of
k_insert_first (DESIGN.md section 4 finding 21), made with the helpers of tests/insert_clean_reads.py.

The sets (two partitions of each kind, reads shuffled):
  groups-G   G in 1, 2, 16, 17: G loci (centres) of one partition; of each an 8-k-mer read, the same read again and a 3-k-mer read
             inside it.  One head per core-key group: one round.  16 groups are 128 instances, table-free; 17 are more heads than
             the fold takes: the sequential fold runs and the partition takes the table path
  slot       two loci whose core keys fall into one slot of the 64 (fold_group_rules.slot), each with a contained read: two rounds
  chain      one locus read as k-mers [0, 16), [8, 24), [16, 32) -- three heads of one group, not clean -- beside a whole copy of
             another locus
  twoheads   one locus as [0, 20) and [10, 30), and [12, 18) which both contain: it folds into the earlier head, not clean
  rec64      exactly 64 records: three whole copies and 61 reads inside them
  i192, i193 192 and 193 instances after the fold (insert_clean_reads' folds-S): the last one k_insert_first takes, the first it leaves

`python insert_fold_groups_worker.py`: every set into a fresh index and into a saturating one, each compared with the oracle's (full
enumeration, nb_kmers, nb_buckets, digest); the conventions of tests/insert_clean_worker.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import insert_clean_reads as R
import fold_group_rules as G

SETS = ("groups-1", "groups-2", "groups-16", "groups-17", "slot", "chain", "twoheads", "rec64", "i192", "i193")
_sets = {}


def _locus_reads(cr, part, spans, copy=None):
    """the reads over `spans` of one locus of the partition (a fresh one where none is given)"""
    def make():
        c = copy if copy is not None else cr.copies(part, 1)[0]
        return [cr.read(c, a, n, part) for a, n in spans], c
    return cr.until(make)[0]


def _groups(cr, count):
    part, reads, cks = cr.partition(), [], set()
    while len(cks) < count:
        got = _locus_reads(cr, part, [(0, 8), (0, 8), (3, 3)])
        if _ck(cr, got[0]) not in cks:  # (two centres of one hash would be one group)
            cks.add(_ck(cr, got[0]))
            reads += got
    return reads


def _ck(cr, copy):
    c, bucket, n, idx0 = cr.O.records(cr.h, copy, R.K, R.M, R.B)
    big = sum(int(w) << (64 * t) for t, w in enumerate(c[0]))
    return G.frames([(int(bucket[0]), int(idx0[0]), int(n[0]), big)])[0]["ck"]


def _slot(cr):
    part, seen = cr.partition(), {}
    while True:
        c = cr.copies(part, 1)[0]
        ck = _ck(cr, c)
        other = seen.setdefault(G.slot(ck), (ck, c))
        if other[0] != ck:
            try:
                return [r for copy in (c, other[1]) for r in _locus_reads(cr, part, [(0, 43), (5, 12)], copy)]
            except AssertionError:  # (a copy that does not take the partial read: on with other pairs)
                pass


def _chain(cr):
    part = cr.partition()
    return _locus_reads(cr, part, [(0, 16), (8, 16), (16, 16)]) + cr.copies(part, 1)


def _twoheads(cr):
    return _locus_reads(cr, cr.partition(), [(0, 20), (10, 20), (12, 6)])


def _rec64(cr):
    part = cr.partition()
    cs, inner = cr.copies(part, 3), []
    for _ in range(4000):  # (a read that begins inside a copy may be given another minimizer: those are passed over)
        r = cr.read(cs[len(inner) % 3], int(cr.rng.integers(0, 30)), int(cr.rng.integers(1, 13)), part)
        if r is not None:
            inner.append(r)
        if len(inner) == 40:
            return cs + inner + inner[:21]
    raise AssertionError("no 40 reads inside three copies")


def _build():
    if _sets:
        return
    cr = R.Crafter(2024)
    try:
        for count in (1, 2, 16, 17):
            _sets[f"groups-{count}"] = R._shuffled(cr, [_groups(cr, count) for _ in range(2)])
        for name, make in (("slot", _slot), ("chain", _chain), ("twoheads", _twoheads), ("rec64", _rec64)):
            _sets[name] = R._shuffled(cr, [make(cr) for _ in range(2)])
        _sets["i192"] = R._shuffled(cr, [R._folds(cr, 192) for _ in range(2)])
        _sets["i193"] = R._shuffled(cr, [R._folds(cr, 193) for _ in range(2)])
    finally:
        cr.close()


def get(name):
    """(flat, offsets) of a set"""
    _build()
    return _sets[name]


def rules_census(O, reads):
    """per partition, from both restated rules (which must agree): records, rounds of either rule, heads, whether the grouped
    rule fell back, instances after the fold, lean, clean"""
    states = {}
    for p, recs in G.partitions_of(O, reads).items():
        if len(recs) > 64:
            states[p] = {"records": len(recs), "lean": False, "clean": False}
            continue
        fr = G.frames(recs)
        s, g = G.sequential(fr), G.grouped(fr)
        assert (s[0], s[1]) == (g[0], g[1]), (p, s, g)
        inst = sum(r[2] for r, (folded, _, _) in zip(recs, s[0]) if not folded)
        lean = inst <= 192
        states[p] = {"records": len(recs), "seq_rounds": s[2], "rounds": g[2], "heads": g[3], "fell_back": g[4], "instances": inst, "lean": lean,
                     "clean": lean and s[1], "slots": len({G.slot(f["ck"]) for f in fr}), "groups": len({f["ck"] for f in fr})}
    return states


def main(B_, O):
    from insert_lean3_worker import Want, check, new_index, out, stage

    for name in SETS:
        reads = get(name)
        want = Want(O, [reads])
        for mode, kw in (("", {}), ("sat-", {"count_mode": "saturate"})):
            with new_index(B_, **kw) as ix:
                stage(mode + name)
                ix.insert_flat(*reads)
                out(mode + name, check(ix, want, f"set {mode}{name}"))


if __name__ == "__main__":
    import brisk_amd
    import oracle

    oracle.build(ref=False)
    main(brisk_amd, oracle.Oracle())
    print("ok")
