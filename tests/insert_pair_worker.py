"""Worker of tests/test_insert_pair.py: one process per environment (the library reads BRISK_INSERT_PAIR and BRISK_DEBUG_INSERT once).
`python insert_pair_worker.py`; stages are announced on stderr as `[lean] stage NAME`, results go to stdout as `NAME <json>` lines,
the last line is `ok` (the conventions of tests/insert_lean3_worker.py).  Every index is compared with the oracle's here: the full
enumeration (k-mer, minimizer_idx, count), nb_kmers, nb_buckets and the digest.  A result is {digest, touched, cnt, cap}: the touched
list in the order the insert kernels walked it, and the directory's (entries, capacity) of those partitions."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

import oracle
import insert_pair_reads as PR
from density_reads import dense_reads, _offsets
from insert_lean3_worker import Want, check, new_index, out, stage

MEDIUM_READS, MEDIUM_GENOME = 20000, 24000  # synthetic reads: about 12 records per touched partition at 2^24 partitions (the error-bearing ones spread over three times as many)


def medium(O, name):
    if name == "medium-synthetic":
        syn = O.synth_reads(MEDIUM_GENOME, 0, MEDIUM_READS)
        return np.ascontiguousarray(syn.reshape(-1)), _offsets(np.full(MEDIUM_READS, syn.shape[1], np.int64))
    return dense_reads(MEDIUM_READS, PR.K, MEDIUM_GENOME, 1, e=0.01)


MEDIUM = ("medium-synthetic", "medium-errors")


def run(B_, O, name, reads, **kw):
    want = Want(O, [reads])
    with new_index(B_, **kw) as ix:
        stage(name)
        ix.insert_flat(*reads)
        touched = ix.debug_touched()
        digest = check(ix, want, name)
        cnt, cap = ix.debug_directory(touched)
        out(name, {"digest": digest, "touched": touched.tolist(), "cnt": cnt.tolist(), "cap": cap.tolist()})


def main(B_, O):
    for name in PR.CASES:
        run(B_, O, name, PR.pack(PR.case(name)))
    for name in PR.SAT_CASES:
        run(B_, O, "sat-" + name, PR.pack(PR.case(name)), count_mode="saturate")
    for name in MEDIUM:
        run(B_, O, name, medium(O, name))


if __name__ == "__main__":
    import brisk_amd

    oracle.build(ref=False)
    main(brisk_amd, oracle.Oracle())
    print("ok")
