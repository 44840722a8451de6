"""Worker of tests/test_sharded.py: one process per environment (the library reads BRISK_INSERT_GENERIC, BRISK_QUERY_GENERIC,
BRISK_HUGE_AT, BRISK_HUGE_QUERY_AT and BRISK_CLS_BITS once per process), a three-owner job through tests/sharded_job.py against the
oracle.  Prints "ok <n checks>"; any mismatch is an AssertionError and exit status 1.

  variants   count and get at (63, 21, 14), (31, 15, 14), (31, 11, 11) and (47, 15, 10), a hot partition among the reads
  cls        BRISK_CLS_BITS=3 at (31, 11, 11): the layout (a 25-bit routing id, 2^25 partitions), the scanned records' routing ids
             against the oracle's, count and get with equal ranges and with cut points on partitions that hold records"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # before the library: torch's HIP runtime first, as in the test process

import brisk_amd
import sharded_cases as C
import sharded_job as S


def count_and_get(reads, queries, k, m, b, n_owners, **kw):
    with S.run(brisk_amd, reads, k, m, b, n_owners, **kw) as job:
        E = job.check()
        assert np.array_equal(S.get(brisk_amd, job, queries), E.query(queries)), (k, m, b, kw, "get")
        return job.records, job.layout


def variants():
    reads, queries = C.variant_reads()
    checks = 0
    for k, m, b in C.VARIANT_GEOMETRIES:
        count_and_get(reads, queries, k, m, b, 3)
        checks += 2
    return checks


def cls():
    env = int(os.environ["BRISK_CLS_BITS"])
    k, m, b = C.CLS3_GEOMETRY
    reads, queries = C.base_reads(), C.base_queries()
    rec, lay = count_and_get(reads, queries, k, m, b, 3)
    want = S.layout_of(k, m, b, 0, env)
    assert (lay["cls_bits"], lay["ext_bits"], lay["part_bits"]) == (want["cls_bits"], want["ext_bits"], want["part_bits"]) == (3, 3, 25), lay
    part, n, _ = S.oracle_partitions(reads, k, m, b, 0, env)
    assert S.same_rows(np.stack([S.partitions(rec, lay, b), S.instances(rec)], axis=1), np.stack([part, n], axis=1)), "routing ids"
    cuts = S.cuts_at_records(part, lay["part_bits"], 3)
    assert 0 < cuts[1] < cuts[2]
    count_and_get(reads, queries, k, m, b, 3, cuts=cuts)
    return 4


if __name__ == "__main__":
    assert torch.cuda.is_available()
    print("ok", {"variants": variants, "cls": cls}[sys.argv[1]]())
