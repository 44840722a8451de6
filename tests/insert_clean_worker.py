"""Worker of tests/test_insert_clean.py: one process per environment (the library reads BRISK_INSERT_CLEAN once).
`python insert_clean_worker.py`; stages are announced on stderr as `[lean] stage NAME`, results go to stdout as `NAME <json>` lines,
the last line is `ok` (the conventions of tests/insert_lean3_worker.py).  Every index is compared with the oracle's here: the full
enumeration (k-mer, minimizer_idx, count), nb_kmers, nb_buckets and the digest."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import oracle
import insert_clean_reads as R
from insert_lean3_worker import Want, check, new_index, out, stage
from saturate_worker import check_index

K, M, B = R.K, R.M, R.B


def main(B_, O):
    # each set alone into a fresh index; the sets whose counts stay far below 255 again into a saturating one (the SAT instantiation)
    for name in R.SETS:
        reads = R.get(name)
        want = Want(O, [reads])
        with new_index(B_) as ix:
            stage(name)
            ix.insert_flat(*reads)
            out(name, check(ix, want, f"set {name}"))
        if name in ("folds", "mixed"):
            with new_index(B_, count_mode="saturate") as ix:
                stage("sat-" + name)
                ix.insert_flat(*reads)
                out("sat-" + name, check(ix, want, f"set {name}, saturating"))
    # a 15-k-mer read 300 times over a clean partition, among twelve clean partitions: 255 for its k-mers (1 + 300 occurrences), the
    # oracle's counts (which wrap) for everything else
    calm, copies, hot = R.hot()
    lines, _, nb = O.count([r.decode() for r in R.hot_reads(1)], K, M, B)
    want = {(w[0], int(w[1])): int(w[2]) for w in (l.split() for l in lines)}
    hot_ids = {(w[0], int(w[1])) for w in (l.split() for l in O.count([hot.decode()], K, M, B)[0])}
    assert len(hot_ids) == 15 and all(want[i] == 2 for i in hot_ids)
    for ident in hot_ids:
        want[ident] = 255
    with B_.BriskHip(K, M, B, immediate_inserts=True, count_mode="saturate") as ix:
        stage("sat-hot")
        ix.insert_reads([r.decode() for r in R.hot_reads(300)])
        check_index(ix, want, nb, K, "a 15-k-mer read x 300 over a clean partition, saturating")
        out("sat-hot", list(ix.checksum()))


if __name__ == "__main__":
    import brisk_amd

    oracle.build(ref=False)
    main(brisk_amd, oracle.Oracle())
    print("ok")
