"""Worker of tests/test_insert_lean3.py: one process per environment (the library reads BRISK_INSERT_LEAN and BRISK_DEBUG_INSERT
once).  `python insert_lean3_worker.py SCENARIO`; stages are announced on stderr as `[lean] stage NAME`, results go to stdout as
`NAME <json>` lines, the last line is `ok` (the conventions of tests/insert_lean_worker.py).  Every index is compared with the
oracle's here: the full enumeration (k-mer, minimizer_idx, count), nb_kmers, nb_buckets and the digest."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import oracle
import insert_lean3_reads as R
from density_reads import as_strings, concat_reads
from saturate_worker import check_index

K, M, B = R.K, R.M, R.B


def stage(name):
    sys.stderr.write(f"[lean] stage {name}\n")
    sys.stderr.flush()


def out(name, value):
    print(name, json.dumps(value), flush=True)


class Want:
    def __init__(self, O, parts):
        flat, offs = concat_reads(parts)
        h = O.index_new(K, M, B)
        try:
            O.index_insert_reads(h, flat, offs)
            self.nk, self.nb = O.index_stats(h)
            lo, hi, idx, cnt = O.index_dump(h)
            self.lines = oracle.multiset_lines(lo, hi, idx, cnt, K)
            self.digest = list(O.digest_entries(lo, hi, idx, cnt))
        finally:
            O.index_free(h)


def check(ix, want, what):
    got = oracle.multiset_lines(*ix.enumerate(), K)
    st = ix.stats()
    assert (st["nb_kmers"], st["nb_buckets"]) == (want.nk, want.nb), (what, st, want.nk, want.nb)
    assert got == want.lines, what
    ck = list(ix.checksum())
    assert ck == want.digest, (what, ck, want.digest)
    return ck


def new_index(B_, **kw):
    ix = B_.BriskHip(K, M, B, immediate_inserts=True, **kw)
    lay = ix.layout
    assert (lay["part_bits"], lay["ext_bits"], lay["record_words"]) == (24, 0, 4), lay
    return ix


def first_batches(B_, O):
    """each set alone into a fresh index"""
    for name, reads in (("one", R.set_one()), ("two", R.set_two())):
        want = Want(O, [reads])
        with new_index(B_) as ix:
            stage(name)
            ix.insert_flat(*reads)
            out(name, check(ix, want, f"set {name}, first batch"))


def scenario_main(B_, O):
    first_batches(B_, O)
    # a second batch into the same index: the general route
    one, two = R.set_one(), R.set_two()
    with new_index(B_) as ix:
        stage("one-again")
        ix.insert_flat(*one)
        stage("second")
        ix.insert_flat(*two)
        out("second", check(ix, Want(O, [one, two]), "set two after set one"))
    # saturating counts.  Set one as it is (the three-slot partitions through the saturating body: every count is 1 or little more,
    # so the oracle's are exact), then one copy of a 192-k-mer locus read 300 times among that locus's reads and sparse ones:
    # 255 for the 43 k-mers of the copy, 1 for the locus's other 149.
    with new_index(B_, count_mode="saturate") as ix:
        stage("sat-one")
        ix.insert_flat(*one)
        check(ix, Want(O, [one]), "set one, saturating")
    locus, copy = R.hot_locus()
    locus = [r.decode() for r in locus]
    sparse = as_strings(*one)[:600]  # (background reads: the loci's come after them)
    lines, _, nb = O.count(sparse + locus, K, M, B)
    want = {(w[0], int(w[1])): int(w[2]) for w in (l.split() for l in lines)}
    hot = {(w[0], int(w[1])) for w in (l.split() for l in O.count([copy.decode()], K, M, B)[0])}
    assert len(hot) == R.W1 and all(want[i] == 1 for i in hot)
    for ident in hot:
        want[ident] = 255
    with B_.BriskHip(K, M, B, immediate_inserts=True, count_mode="saturate") as ix:
        stage("sat-hot")
        ix.insert_reads(sparse[:300] + locus + [copy.decode()] * 299 + sparse[300:])
        check_index(ix, want, nb, K, "one copy of a 192-k-mer locus x 300, saturating")


if __name__ == "__main__":
    import brisk_amd

    oracle.build(ref=False)
    {"main": scenario_main, "first-batches": first_batches}[sys.argv[1]](brisk_amd, oracle.Oracle())
    print("ok")
