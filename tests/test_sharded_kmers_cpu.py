"""Without a device: the entry points of the sharded per-k-mer get are declared and exported, the split arithmetic of the answers'
return trip is right, and the cases of tests/test_sharded_kmers.py are not vacuous -- shown from the oracle alone: at least two
owners own records with present k-mers, both vector orientations occur among the queries, and some records hold nothing but
absent k-mers."""
import os
import random
import re

import numpy as np
import pytest

import sharded_cases as C
import sharded_job as S
import sharded_kmers_job as K
from brisk_amd import exchange as X
from brisk_amd import hipapi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["brisk_hip_scan_kmers", "brisk_hip_record_kmers", "brisk_hip_answer_records", "brisk_hip_place_answers", "brisk_hip_profile_slots"]


def test_the_five_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    L = hipapi.load()
    for s in NEW:
        assert s in hipapi.SYMBOLS
        assert re.search(r"^int %s\(brisk_hip_index \*h," % s, header, re.M), s
        assert hasattr(L, s), s
        assert "no reference counterpart" in header[header.index(s):][:400], s  # (the reference table at the top)
    assert "#define BRISK_HIP_ABI_VERSION 4" in header and L.brisk_hip_abi_version() == 4
    for s in ("scan_kmers", "record_kmers", "answer_records", "place_answers", "profile_slots"):
        assert callable(getattr(hipapi.BriskHip, s))
    for s in ("get_kmers_packed", "read_profile_packed", "trim_packed", "count_spectrum", "prune", "checksum"):
        assert callable(getattr(X.ShardedCounter, s))


def test_answer_splits():
    """the answers owed per group of records are the differences of the record_kmers table at the group boundaries"""
    import torch
    rng = random.Random(5)
    assert X.answer_splits(np.array([0]), [0, 0, 0]) == [0, 0, 0]
    assert X.answer_splits(np.array([0, 3, 5, 5, 9]), [2, 0, 2]) == [5, 0, 4]
    for _ in range(200):
        world = rng.randint(1, 9)
        counts = [rng.choice([0, 0, 1, rng.randint(0, 40)]) for _ in range(world)]
        n = [rng.randint(0, 255) for _ in range(sum(counts))]  # (a record without k-mers does not occur, and does not hurt)
        offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
        want, at = [], 0
        for c in counts:
            want.append(sum(n[at:at + c]))
            at += c
        assert X.answer_splits(offsets, counts) == want
        assert X.answer_splits(torch.from_numpy(offsets.astype(np.int64)), counts) == want
        assert sum(want) == int(offsets[-1])
    # past 2^32 answers: the table is 64-bit
    big = np.array([0, 1 << 33, (1 << 33) + 7], np.uint64)
    assert X.answer_splits(big, [1, 1]) == [1 << 33, 7]


def equal_or(cuts, part_bits, n_owners):
    return cuts if cuts is not None else X.uniform_cuts(part_bits, n_owners)


@pytest.mark.parametrize("k,m,b", K.KMER_GEOMETRIES)
def test_round_trip_cases(O, k, m, b):
    reads, queries = C.base_reads(), C.base_queries()
    f = K.facts(reads, queries, k, m, b)
    for name, n in K.CUT_SCHEMES:
        cuts = equal_or(K.cuts_of(name, n, reads, k, m, b), f["part_bits"], n)
        assert len(cuts) == n + 1
        K.assert_not_vacuous(f, cuts, (k, m, b, name, n))
        if name == "balanced":
            assert cuts != X.uniform_cuts(f["part_bits"], n), (k, m, b, n)
    # shorter than k, and empty: reads without slots among the queries
    assert any(len(q) == 0 for q in queries) and any(0 < len(q) < k for q in queries)


@pytest.mark.parametrize("row", C.EDGE_ROWS, ids=C.row_id)
def test_boundary_cases(O, row):
    f = K.facts(C.edge_reads(row), C.edge_queries(row), row.k, row.m, row.b, row.part_bits)
    K.assert_not_vacuous(f, X.uniform_cuts(f["part_bits"], 3), C.row_id(row))


@pytest.mark.parametrize("k,m,b", C.LONG_GEOMETRIES)
def test_long_sequence_cases(O, k, m, b):
    seqs, queries = C.long_sequences()
    f = K.facts(seqs, queries, k, m, b)
    K.assert_not_vacuous(f, X.uniform_cuts(f["part_bits"], 3), (k, m, b, "long"))
    assert sum(len(q) - k + 1 > 8192 for q in queries) >= 5  # the chunked scan


@pytest.mark.parametrize("k,m,b", C.VARIANT_GEOMETRIES)
def test_variant_cases(O, k, m, b):
    reads, queries = C.variant_reads()
    f = K.facts(reads, queries, k, m, b)
    K.assert_not_vacuous(f, X.uniform_cuts(f["part_bits"], 3), (k, m, b, "variants"))


@pytest.mark.parametrize("k,m,b", C.COUNT_GEOMETRIES)
def test_wrapped_count_cases(O, k, m, b):
    reads, queries, hot = K.wrap_case(k)
    f = K.facts(reads, queries, k, m, b)
    K.assert_not_vacuous(f, X.uniform_cuts(f["part_bits"], 3), (k, m, b, "wrap"))
    want, _, base = K.expected(reads, queries, k, m, b)
    assert len(hot) == k + 20 and (want[int(base[0]):int(base[1])] == 0x100).all()  # 256 times: present, count 0
    rest = want[int(base[1]):]
    assert ((rest & 0xff) < 255).all()  # nothing else comes near 255: the saturating index differs in the hot read alone


@pytest.mark.parametrize("k,m,b", K.PROFILE_GEOMETRIES)
def test_profile_cases(O, k, m, b):
    """solid_min 0, 2 and 300 tell the reads apart, and under BRISK_PROFILE_SEG=64 the 150 nt reads are reduced in segments"""
    reads, queries = C.base_reads(), C.base_queries()
    want, _, base = K.expected(reads, queries, k, m, b)
    p0, p2, p300 = (K.expected_profile(want, base, s) for s in K.SOLID_MINS)
    assert (p300["n_solid"] == 0).all() and (p0["n_solid"] == p0["n_present"]).all()
    assert (p2["n_solid"] < p0["n_solid"]).any() and (p2["n_solid"] > 0).any()
    assert (p0["n_kmers"] > 64).sum() > 100 and (p0["n_kmers"] == 0).any()


@pytest.mark.parametrize("k,m,b", C.RANKS_GEOMETRIES)
def test_four_rank_cases(O, k, m, b):
    everything = [s for i in range(len(C.RANK_SHARES)) for r in range(4) for s in C.rank_reads(i, r)]
    lay = S.layout_of(k, m, b)
    cuts = X.uniform_cuts(lay["part_bits"], 4)
    n_batches = []
    for rank in range(4):
        queries = K.rank_queries(rank)
        n_batches.append((len(queries) + K.RANK_BATCH_READS - 1) // K.RANK_BATCH_READS)
        if queries:
            K.assert_not_vacuous(K.facts(everything, queries, k, m, b), cuts, (k, m, b, "rank", rank))
    assert max(n_batches) >= 2 and n_batches[2] < max(n_batches), n_batches  # several agreed batches, rank 2 idle in one
    E = S.expect(everything, k, m, b)
    cnt = np.asarray(E.dump[3])
    assert (cnt == 1).sum() > 100 and (cnt >= 2).sum() > 100  # prune(2, 255) removes some entries and keeps some
