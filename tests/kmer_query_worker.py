"""Worker of test_kmer_query.py::test_kernel_variants_match_the_oracle: one process per environment (the library reads
BRISK_BINS, BRISK_QUERY_GENERIC, BRISK_HUGE_QUERY_AT, BRISK_QUERY_ENT once); the per-k-mer get against the oracle.
Prints "ok <n checks>"."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # before the library: torch's HIP runtime first, as in the test process

import brisk_amd
import oracle
from test_gpu_parity import _random_reads
from test_kmer_query import GEOMETRIES, as_u16, assert_slots, expected_all, get_kmers_packed, oracle_index, query_set

assert torch.cuda.is_available()
oracle.build(ref=False)
O = oracle.Oracle()
checks = 0
for k, m, b in GEOMETRIES:
    rng = random.Random(k + m + b)
    reads = _random_reads(rng, 1500, 300) + ["A" * 150] * 40 + ["ACGT" * 40] * 3
    queries = query_set(rng, reads, k)
    h = oracle_index(O, reads, k, m, b)
    want, alts, base = expected_all(O, h, queries, k, m)
    O.index_free(h)
    with brisk_amd.BriskHip(k, m, b) as ix:
        ix.insert_reads(reads)
        counts, found, got_base = ix.get_kmers(queries)
        assert np.array_equal(got_base, base)
        got = as_u16(counts, found)
        assert_slots(got, want, alts, (k, m, b, os.environ.get("BRISK_BINS")))
        assert np.array_equal(get_kmers_packed(brisk_amd, ix, queries), got), (k, m, b, "packed")
    checks += 1
print(f"ok {checks}")
