"""Worker of tests/test_sharded_kmers.py: one process per environment (the library reads BRISK_QUERY_GENERIC, BRISK_HUGE_QUERY_AT,
BRISK_INSERT_GENERIC, BRISK_HUGE_AT and BRISK_PROFILE_SEG once per process), a three-owner job through tests/sharded_kmers_job.py
against the oracle.  Prints "ok <n checks>"; any mismatch is an AssertionError and exit status 1.

  variants   the per-k-mer round trip at (63, 21, 14), (31, 15, 14), (31, 11, 11) and (47, 15, 10), a hot partition among the reads
  segments   the round trip, profile_slots and the rules at the profile geometries (run under BRISK_PROFILE_SEG=64)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # before the library: torch's HIP runtime first, as in the test process

import brisk_amd
import sharded_cases as C
import sharded_kmers_job as K


def variants():
    reads, queries = C.variant_reads()
    for k, m, b in C.VARIANT_GEOMETRIES:
        K.check_case(brisk_amd, reads, queries, k, m, b, 3)
    return len(C.VARIANT_GEOMETRIES)


def segments():
    assert os.environ["BRISK_PROFILE_SEG"] == "64"
    for k, m, b in K.PROFILE_GEOMETRIES:
        K.check_case(brisk_amd, C.base_reads(), C.base_queries(), k, m, b, 3, profiles=True)
    return len(K.PROFILE_GEOMETRIES)


if __name__ == "__main__":
    assert torch.cuda.is_available()
    print("ok", {"variants": variants, "segments": segments}[sys.argv[1]]())
