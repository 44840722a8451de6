"""Without a device: the cases of tests/test_sharded.py are not vacuous, shown from the oracle's records alone, and the owner
arithmetic tests/sharded_job.py checks the device against agrees with the three functions of brisk_amd.exchange."""
import random

import numpy as np
import pytest

import sharded_cases as C
import sharded_job as S
from brisk_amd import exchange as X


def held(part, cuts):
    """records per owner"""
    return np.bincount(S.owner_of(part, cuts), minlength=len(cuts) - 1)


def spread(part, cuts, what):
    """every owner with partitions receives records, every owner without receives none, and at least two a tenth of them"""
    h = held(part, cuts)
    for o in range(len(cuts) - 1):
        assert (h[o] > 0) == (cuts[o + 1] > cuts[o]), (what, "owner %d" % o, h.tolist(), cuts)
    assert (h * 10 >= len(part)).sum() >= min(2, sum(cuts[o + 1] > cuts[o] for o in range(len(cuts) - 1))), (what, h.tolist())
    return h


def test_owner_arithmetic_agrees_with_the_exchange_module():
    rng = random.Random(77)
    for _ in range(300):
        pb = rng.randint(1, 30)
        N = rng.randint(1, min(256, 1 << pb))
        uni = X.uniform_cuts(pb, N)
        # uniform_cuts[o] is the smallest partition whose owner is o
        assert all((uni[o] * N) >> pb >= o and (o == 0 or ((uni[o] - 1) * N) >> pb < o) for o in range(N)) and uni[N] == 1 << pb, (pb, N)
        part = np.array([rng.randrange(1 << pb) for _ in range(200)] + [0, (1 << pb) - 1] + [c for c in uni[:-1]] + [c - 1 for c in uni[1:]], dtype=np.int64)
        want = (part * N) >> pb
        assert np.array_equal(S.owner_of(part, uni), want), (pb, N)
        assert np.array_equal(X.owner_of_partition(part, uni), want), (pb, N)
        b = rng.randint((pb + 1) // 2, 16) if pb <= 32 and (pb + 1) // 2 <= 16 else 16
        ext = rng.randint(0, min(4, 32 - 2 * b)) if 2 * b == pb else 0  # an extended routing id is never cut; it has at most 32 bits
        shift = 2 * b + ext - pb
        rid = (part << shift) | np.array([rng.randrange(1 << shift) for _ in part], dtype=np.int64)
        assert np.array_equal(X.owner_of_bucket(rid, b, pb, N, ext_bits=ext), want), (pb, N, b, ext)
        rec = np.zeros((len(rid), 2), np.uint64)  # records of two words: the header is the last, n and idx0 above the routing id
        rec[:, 1] = rid.astype(np.uint64) | np.uint64((7 << 32) | (9 << 40))
        assert np.array_equal(S.partitions(rec, dict(ext_bits=ext, part_bits=pb), b), part)
        # cut points with repeats (owners without partitions)
        cuts = [0] + sorted(rng.choice([rng.randrange(1 << pb), int(rng.choice(part))]) for _ in range(N - 1)) + [1 << pb]
        o = S.owner_of(part, cuts)
        assert np.array_equal(o, X.owner_of_partition(part, cuts)), (pb, N, cuts)
        lo, hi = np.asarray(cuts)[o], np.asarray(cuts)[o + 1]
        assert ((lo <= part) & (part < hi)).all()


@pytest.mark.parametrize("k,m,b", C.COUNT_GEOMETRIES)
def test_owner_count_cases(O, k, m, b):
    reads, queries = C.base_reads(), C.base_queries()
    part, n, lay = S.oracle_partitions(reads, k, m, b)
    for N in C.OWNER_COUNTS:
        spread(part, X.uniform_cuts(lay["part_bits"], N), (k, m, b, N))
    if (k, m, b) == (31, 11, 4):
        assert (lay["part_bits"], lay["ext_bits"], lay["cls_bits"]) == (23, 15, 1) and len(part) > len(reads) * 8
    # balanced cuts from the job's histogram differ from the equal ranges, and every owner still receives records
    hist = np.zeros(1 << lay["part_bits"], np.int64)
    np.add.at(hist, part, 1 + (n << 32))
    import torch
    cuts = X.balanced_cuts(torch.from_numpy(hist), lay["part_bits"], 8)
    assert cuts != X.uniform_cuts(lay["part_bits"], 8)
    spread(part, cuts, (k, m, b, "balanced"))
    # the queries: present k-mers (reads of the job) and absent ones (reads of another genome)
    want = S.expect(reads, k, m, b).query(queries)
    n_special = len(queries) - 150 - 100 - 12
    assert (want[:150] > 0).all() and (want[150 + n_special:150 + n_special + 100] == 0).all()
    # pieces = 3 and the second batch: every piece of every rank has reads
    assert len(reads) // 3 // 3 > 100


@pytest.mark.parametrize("row", C.EDGE_ROWS, ids=C.row_id)
def test_boundary_geometry_cases(O, row):
    reads = C.edge_reads(row)
    part, n, lay = S.oracle_partitions(reads, row.k, row.m, row.b, row.part_bits)
    spread(part, X.uniform_cuts(lay["part_bits"], 3), (C.row_id(row), "equal"))
    cuts = S.cuts_at_records(part, lay["part_bits"], 3)
    assert 0 < cuts[1] < cuts[2] < 1 << lay["part_bits"]
    h = spread(part, cuts, (C.row_id(row), "cuts"))
    assert set(cuts[1:3]) <= set(part.tolist())  # the cuts fall on partitions that hold records
    want = S.expect(reads, row.k, row.m, row.b).query(C.edge_queries(row))
    assert (want[:70] > 0).all() and (want == 0).any()
    assert h.min() * 5 >= len(part)


def test_smallest_geometry_with_eight_equal_owners(O):
    """(12, 5, 1): 2^11 partitions from a 2-bit bucket id, 8 hash bits and a class bit.  Eight equal owners are the bucket and the
    TOP bit of the minimizer's hash: minimizers are the smallest hashes of their windows, so the owners with that bit set hold
    less -- but none holds nothing.  Four owners come out empty only when the owner is taken from the bucket id alone, that is,
    with the routing id's ext_bits forgotten (the mistake sharded_job's range invariant is written against)."""
    row = C.SMALLEST
    part, n, lay = S.oracle_partitions(C.edge_reads(row), row.k, row.m, row.b)
    assert (lay["part_bits"], lay["ext_bits"]) == (11, 9)
    uni = X.uniform_cuts(11, 8)
    h = held(part, uni)
    assert h.min() > 0 and (h * 10 >= len(part)).sum() >= 2, h.tolist()
    assert h[0::2].min() > h[1::2].max(), h.tolist()
    assert (held((part >> 9) << 9, uni) == 0).sum() == 4


@pytest.mark.parametrize("row", C.EMPTY_OWNER_ROWS, ids=C.row_id)
def test_empty_owner_cases(O, row):
    part, n, lay = S.oracle_partitions(C.edge_reads(row), row.k, row.m, row.b, row.part_bits)
    end, c = 1 << lay["part_bits"], C.middle_cut(row)
    assert 0 < c < end and c in set(part.tolist())
    for cuts in ([0, 0, c, end], [0, c, c, end], [0, c, end, end]):
        spread(part, cuts, (C.row_id(row), cuts))
    for cuts in ([0, end, end, end], [0, 0, end, end], [0, 0, 0, end]):
        h = held(part, cuts)
        assert sorted(h.tolist()) == [0, 0, len(part)]


def test_three_class_bits_case(O):
    k, m, b = C.CLS3_GEOMETRY
    part, n, lay = S.oracle_partitions(C.base_reads(), k, m, b, 0, 3)
    assert (lay["cls_bits"], lay["part_bits"], 2 * b + lay["ext_bits"]) == (3, 25, 25)
    spread(part, X.uniform_cuts(25, 3), "cls equal")
    spread(part, S.cuts_at_records(part, 25, 3), "cls cuts")
    assert len(set((part & 7).tolist())) >= 5  # classes that need the third bit occur


@pytest.mark.parametrize("k,m,b", C.MANY_OWNER_GEOMETRIES)
def test_many_owner_cases(O, k, m, b):
    reads = C.many_owner_reads(k, m, b)
    part, n, lay = S.oracle_partitions(reads, k, m, b)
    pb = lay["part_bits"]
    assert 256 <= 1 << pb
    h = held(part, X.uniform_cuts(pb, 256))
    assert (h > 0).sum() >= 16, (h > 0).sum()
    assert min(h[0], h[127], h[255]) > 0, h[[0, 127, 255]].tolist()  # the three owners that test_many_owners fills
    for seed in (1, 2):
        cuts = C.random_cuts(seed, part, pb, 256)
        assert len(cuts) == 257 and cuts == sorted(cuts) and len(set(cuts)) < 257  # repeats: owners without partitions
        hc = held(part, cuts)
        assert (hc > 0).sum() >= 8
        assert len(set(cuts[1:-1]) & set(part.tolist())) >= 100  # cuts ON partitions that hold records


def test_refusal_case(O):
    row = C.SIXTY_FOUR_PARTITIONS
    assert 1 << S.layout_of(row.k, row.m, row.b, row.part_bits)["part_bits"] == 64 < 65
    assert len(S.oracle_partitions(C.edge_reads(row)[:60], row.k, row.m, row.b, row.part_bits)[0]) > 0


@pytest.mark.parametrize("k,m,b", C.LONG_GEOMETRIES)
def test_long_sequence_case(O, k, m, b):
    seqs, queries = C.long_sequences()
    assert sum(len(s) - k + 1 > 8192 for s in seqs) == 5 and len(seqs) == 205
    part, n, lay = S.oracle_partitions(seqs, k, m, b)
    spread(part, X.uniform_cuts(lay["part_bits"], 3), (k, m, b, "long"))
    want = S.expect(seqs, k, m, b).query(queries)
    # present k-mers (a random sequence finds all of its own) and absent ones (the poly-A queries' random stretches, and where
    # query_sequence stops)
    kmers = np.array([max(0, len(q) - k + 1) for q in queries])
    assert want[0] == kmers[0] and want[1] == kmers[1] and (want[-3:] < kmers[-3:]).all() and want[-3] == 0


def test_kernel_variant_cases(O):
    reads, queries = C.variant_reads()
    for k, m, b in C.VARIANT_GEOMETRIES:
        part, n, lay = S.oracle_partitions(reads, k, m, b)
        spread(part, X.uniform_cuts(lay["part_bits"], 3), (k, m, b, "variants"))
        inst = np.zeros(1 << lay["part_bits"], np.int64)
        np.add.at(inst, part, n)
        # BRISK_HUGE_AT=24: partitions of more than 24 instances exist (the workgroup-per-partition insert), the hot one far above
        assert (inst > 24).sum() >= 10 and inst.max() >= 40 * (150 - k + 1), (k, m, b)
        want = S.expect(reads, k, m, b).query(queries)
        assert (want > 0).any() and (want == 0).any()


def test_four_rank_cases(O):
    """k31 m15 b14: 2000 reads bring more records than six a read (ShardedCounter's estimate), and equal ranges over four owners
    carry more than 1.3 times the mean (so balance() installs cut points without being forced); (31, 11, 4) stays below 1.3."""
    ratio = {}
    for k, m, b in C.RANKS_GEOMETRIES:
        lay = S.layout_of(k, m, b)
        pb = lay["part_bits"]
        inst = np.zeros(1 << pb, np.int64)
        per_rank = []
        for r in range(4):
            reads = [s for i in range(len(C.RANK_SHARES)) for s in C.rank_reads(i, r)]
            part, n, _ = S.oracle_partitions(reads, k, m, b)
            np.add.at(inst, part, n)
            per_rank.append(len(part))
        first = len(S.oracle_partitions(C.rank_reads(0, 0), k, m, b)[0])
        if (k, m, b) == (31, 15, 14):
            assert len(C.rank_reads(0, 0)) == 2000 and first == 26092 > 2000 * 6 + 4096
        uni = X.uniform_cuts(pb, 4)
        load = [int(inst[uni[o]:uni[o + 1]].sum()) for o in range(4)]
        ratio[(k, m, b)] = max(load) * 4 / sum(load)
        assert min(load) * 10 >= sum(load) / 4
    assert ratio[(31, 15, 14)] > 1.3 >= ratio[(31, 11, 4)], ratio
    absent = S.expect([s for i in range(2) for r in range(4) for s in C.rank_reads(i, r)], 31, 15, 14).query(["".join(random.Random(900).choice("ACGT") for _ in range(150))])
    assert absent[0] == 0


def test_saturating_case(O):
    """the saturating job is held to the oracle, whose counts wrap: its reads keep every count far below 255"""
    for k, m, b in C.COUNT_GEOMETRIES:
        E = S.expect(C.saturate_reads(), k, m, b)
        assert 1 < int(E.dump[3].max()) < 128 and len(E.dump[0]) > 1000
        part, n, lay = S.oracle_partitions(C.saturate_reads(), k, m, b)
        spread(part, X.uniform_cuts(lay["part_bits"], 3), (k, m, b, "saturate"))
