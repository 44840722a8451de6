"""The inputs of the sharded tests: geometries, read sets, cut points.  Shared by tests/test_sharded.py, its
workers and tests/test_sharded_cpu.py, which shows from the oracle alone that they are not vacuous.  Nothing here is a test and
nothing touches the device.  (tests/geometry_edges.py, whose table and read sets the boundary rows reuse, imports the low-complexity
reads from tests/test_gpu_parity.py, as tests/geometry_edges_worker.py does outside pytest.)"""
import random

import numpy as np

import geometry_edges as G
from sharded_job import _once, oracle_partitions, the_oracle

SPECIAL = G.SPECIAL


def _random_reads(rng, n, glen, L=150):
    """n reads of L nt from a random genome of glen nt, either strand (test_gpu_parity._random_reads, restated: same draws)"""
    genome = "".join(rng.choice("ACGT") for _ in range(glen))
    out = []
    for _ in range(n):
        p = rng.randrange(0, glen - L)
        s = genome[p:p + L]
        if rng.random() < 0.5:
            s = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
        out.append(s)
    return out


COUNT_GEOMETRIES = [(63, 21, 14), (31, 11, 4)]  # (31, 11, 4): a 23-bit routing id: 8 bucket bits, 14 hash bits and a class bit
OWNER_COUNTS = [2, 3, 5, 7, 8]
LONG_GEOMETRIES = [(63, 21, 14), (31, 11, 11)]
MANY_OWNER_GEOMETRIES = [(12, 5, 1), (63, 21, 14)]
VARIANT_GEOMETRIES = [(63, 21, 14), (31, 15, 14), (31, 11, 11), (47, 15, 10)]
VARIANT_ENVS = [{"BRISK_INSERT_GENERIC": "1", "BRISK_QUERY_GENERIC": "1"}, {"BRISK_HUGE_AT": "24", "BRISK_HUGE_QUERY_AT": "8"},
                {"BRISK_HUGE_AT": "24", "BRISK_HUGE_QUERY_AT": "0"}]
RANKS_GEOMETRIES = [(31, 15, 14), (31, 11, 4)]
RANK_SHARES = [(2000, 700, 0, 300), (0, 50, 900, 0)]  # reads per rank and count_packed batch
CLS3_GEOMETRY = (31, 11, 11)  # under BRISK_CLS_BITS=3: a 25-bit routing id
row_id = G.row_id
_rows = {(r.k, r.m, r.b, r.part_bits): r for r in G.TABLE}
EDGE_ROWS = [_rows[x] for x in ((33, 11, 4, 0), (33, 11, 6, 6), (37, 15, 10, 8), (63, 21, 2, 0), (12, 5, 1, 0), (32, 11, 3, 0))]
SMALLEST, SIXTY_FOUR_PARTITIONS = _rows[(12, 5, 1, 0)], _rows[(33, 11, 6, 6)]
EMPTY_OWNER_ROWS = [SMALLEST, _rows[(37, 15, 10, 8)]]
def base_reads():
    """1500 reads of 150 nt from 4 kb, both strands, the low-complexity set, forty ragged reads of 1-400 nt, an empty one"""
    def make():
        rng = random.Random(2025)
        return _random_reads(rng, 1500, 4000) + SPECIAL + ["".join(rng.choice("ACGT") for _ in range(rng.randint(1, 400))) for _ in range(40)] + ["", "A"]
    return _once("base", make)


def base_queries():
    """reads of the job (present), the low-complexity set, reads of another genome (absent), ragged ones"""
    def make():
        rng = random.Random(2026)
        reads = base_reads()
        return [q.upper() for q in reads[:150] + SPECIAL + _random_reads(rng, 100, 4000) + reads[-12:]]
    return _once("base queries", make)


def saturate_reads():
    """the first 300 random reads of the base set (coverage 11: no count comes near 255, so wrapping and saturating counts agree)"""
    return base_reads()[:300]


def edge_reads(row):
    return _once(("edge", row), lambda: G.read_sets(row))[0]


def edge_queries(row):
    a, b, c = _once(("edge", row), lambda: G.read_sets(row))
    return G.queries_of(a, b, c)


def middle_cut(row):
    """the partition of the median record: a cut point that leaves records on both sides and falls on a partition that holds some"""
    part, _, _ = oracle_partitions(edge_reads(row), row.k, row.m, row.b, row.part_bits)
    return int(np.sort(part)[len(part) // 2])


def many_owner_reads(k, m, b):
    return edge_reads(SMALLEST) if (k, m, b) == (12, 5, 1) else base_reads()


def random_cuts(seed, part, part_bits, n_owners):
    """n_owners + 1 ascending cut points with repeats: two thirds of them drawn from the partitions that hold records (a cut ON such
    a partition tells `<=` from `<`), some of those twice, the rest anywhere"""
    rng = random.Random(seed)
    held = sorted(set(int(p) for p in part))
    inner = [rng.choice(held) for _ in range((n_owners - 1) * 2 // 3)]
    inner += [rng.choice(inner) for _ in range((n_owners - 1) // 6)]
    inner += [rng.randrange(1 << part_bits) for _ in range(n_owners - 1 - len(inner))]
    return [0] + sorted(inner) + [1 << part_bits]


def long_sequences():
    """(sequences, queries): the long sequences of test_chromosome_length_sequences_are_scanned_in_chunks that differ in how their
    chunks' seams behave, 200 short reads in the same batch; the queries add that test's three sequences with poly-A stretches"""
    def make():
        rng = random.Random(2024)
        rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
        seqs = [rnd(8192 + 63), rnd(40_000), "A" * 30_000, "ACGTTGCA" * 4000, rnd(15_000) + "T" * 20_000 + rnd(15_000)]
        seqs += _random_reads(rng, 200, 3000)
        queries = seqs + [rnd(20_000) + "A" * 90 + rnd(20_000), "A" * 70 + rnd(30_000), rnd(9_000) + "A" * 500 + rnd(9_000) + "A" * 64 + rnd(5_000)]
        return seqs, queries
    return _once("long", make)


def variant_reads():
    """(reads, queries) of tests/env_variant_worker.py: a hot partition (forty poly-A reads) among reads of a 300 nt genome"""
    def make():
        rng = random.Random(61)
        reads = _random_reads(rng, 1500, 300) + SPECIAL + ["A" * 150] * 40 + ["ACGT" * 40] * 3
        return reads, reads[:300] + SPECIAL + _random_reads(rng, 200, 300)
    return _once("variant", make)


def rank_reads(batch, rank):
    """the reads of one rank in one count_packed batch of the four-rank job: consecutive reads of Oracle.synth_reads(60000, ...)"""
    first = sum(sum(sh) for sh in RANK_SHARES[:batch]) + sum(RANK_SHARES[batch][:rank])
    n = RANK_SHARES[batch][rank]
    return _once(("rank", batch, rank), lambda: [bytes(r) for r in the_oracle().synth_reads(60000, first, n)] if n else [])
