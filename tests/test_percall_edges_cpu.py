"""CPU: the inputs of tests/test_percall_edges.py and tests/percall_worker.py can tell a right answer from a wrong one -- the
non-vacuity conditions of the per-call protocol's replay (tests/percall_reference.py), from the oracle alone -- and the host side of
the per-call C-ABI that needs no device."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import geometry_edges as G
import percall_reference as P

ROWS = G.TABLE + G.CLS_EXTRA
BIG_PARTITIONS = [G.TABLE[6], G.TABLE[4]]  # (31, 11, 4, pb 2) and (33, 11, 6, pb 6)


@pytest.mark.parametrize("r", ROWS, ids=[G.row_id(r) for r in ROWS])
def test_replay_is_the_oracles_count_and_mixes_found_and_new(O, r):
    rp = P.replay(O, r)
    fig = rp.figures()
    print(G.row_id(r), fig)
    lines, nb_kmers, nb_buckets = P.oracle_count(O, r, rp.seqs)
    assert rp.lines() == lines and len(rp.entries) == nb_kmers and nb_buckets > 1
    assert sorted(rp.id_of.values()) == list(range(len(rp.entries)))
    assert fig["longest"] == r.k - r.m + 1
    assert fig["found"] * 10 >= fig["kmers"] and fig["new"] * 10 >= fig["kmers"]
    assert fig["mixed"] >= 1
    assert max(rp.data) > 3 and min(rp.data) == 1
    assert sum(len(s) < r.k for s in rp.seqs) == 2 and all(len(st[0]) == 0 for s, st in zip(rp.seqs, rp.streams) if len(s) < r.k)
    # the one-bit neighbours of the entries: mostly absent, and the oracle's index agrees with the replay on each
    fl = P.flipped(rp, O, r)
    assert len(fl) == 2 and all((want == P.ABSENT).sum() * 2 > len(want) for *_, want in fl)


@pytest.mark.parametrize("r", BIG_PARTITIONS, ids=[G.row_id(r) for r in BIG_PARTITIONS])
def test_some_partition_ends_above_a_wave(O, r):
    """more than one trip of k_upsert's and k_lookup's 64-lane loops, and slice moves of more than 64 entries"""
    biggest = Counter(P.partitions(O, r, P.replay(O, r))).most_common(1)[0][1]
    assert biggest > 64
    assert P.grow_cap(64) == 88 and P.grow_cap(1) == 9  # n + n / 4 + 8


def test_predict_cursor_by_hand():
    # one partition: slices of grow_cap(1) = 9, grow_cap(10) = 20, grow_cap(21) = 34 slots for 22 entries
    assert P.predict_cursor([5] * 9) == 9 and P.predict_cursor([5] * 10) == 29 and P.predict_cursor([5] * 22) == 63
    assert P.predict_cursor([1, 2, 1, 3]) == 27 and P.predict_cursor([]) == 0


@pytest.mark.parametrize("r", P.GROWTH_ROWS, ids=[G.row_id(r) for r in P.GROWTH_ROWS])
def test_growth_inputs_grow_the_arena_twice_and_resume_a_vector(O, r):
    """the inputs of the BRISK_NO_VMM and BRISK_ARENA_LIMIT runs: the predicted cursor passes 90,000 slots and, replaying the host's
    growth rule, the copy-growth arena grows at least twice beyond its first 65,536 entries, at least once part-way through a vector"""
    rp, parts, growths, cursor = P.growth_case(O, r)
    fig = rp.figures()
    print(G.row_id(r), fig, cursor, growths)
    assert cursor == P.predict_cursor(parts) >= 90_000
    assert len(growths) >= 2 and any(0 < g.done < g.n for g in growths)
    assert [g.arena for g in growths] == sorted({g.arena for g in growths}) and growths[0].arena > P.FIRST_ARENA
    assert 2_000 <= fig["vectors"] <= 12_000 and fig["found"] > 1000
    limit = P.arena_limit(growths)
    refused, _ = P.predict_growths(rp, parts, limit=limit)
    assert len(refused) == 2 and refused[0] == growths[0] and refused[1].arena is None and refused[1][:4] == growths[1][:4]
    lines, nb_kmers, _ = P.oracle_count(O, r, rp.seqs)
    assert rp.lines() == lines and len(rp.entries) == nb_kmers


# ---- the C-ABI's host side -----------------------------------------------------------------------------------------------------
def test_exports_and_the_255_kmer_cap():
    """The per-call entry points are exported with the signatures brisk_amd.hipapi binds, and brisk_hip_upsert_kmers refuses more than
    255 k-mers (a vector has at most k - m + 1 <= 63) from its arguments alone: the check comes before anything looks at the handle,
    so a block of zeros stands in for one here."""
    import brisk_amd
    from brisk_amd import hipapi
    brisk_amd.build_library()
    L = hipapi.load()
    for s in ("brisk_hip_scan_sequence", "brisk_hip_upsert_kmers", "brisk_hip_find_kmers", "brisk_hip_enumerate_ids", "brisk_hip_reallocate",
              "brisk_hip_memory_info"):
        assert s in hipapi.SYMBOLS and hasattr(L, s), s
    EINVAL = 1
    lo, hi, idx = np.zeros(256, np.uint64), np.zeros(256, np.uint64), np.zeros(256, np.uint8)
    ids, new = np.full(256, 7, np.uint32), np.full(256, 7, np.uint8)
    assert L.brisk_hip_upsert_kmers(None, lo, hi, idx, 1, ids, new) == EINVAL
    assert L.brisk_hip_find_kmers(None, lo, hi, idx, 1, ids) == EINVAL
    n = C.c_uint64(5)
    assert L.brisk_hip_scan_sequence(None, b"ACGT", 4, 1, lo, ids, lo, hi, idx, C.byref(n)) == EINVAL
    stand_in = C.create_string_buffer(1 << 16)
    assert L.brisk_hip_upsert_kmers(C.cast(stand_in, C.c_void_p), lo, hi, idx, 256, ids, new) == EINVAL
    assert (ids == 7).all() and (new == 7).all() and stand_in.raw == bytes(1 << 16)
