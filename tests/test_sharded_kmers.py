"""The per-k-mer get, read profiles and trimming across bucket-range shards, on one device against the oracle:
N owners driven through the C-ABI by tests/sharded_kmers_job.py -- scan_kmers, route_tagged, record_kmers, answer_records on each
owner, place_answers -- which asserts the routing, the offset tables, the answer counts and that every slot is written once; the
slots are compared here with test_kmer_query.expected_all over the oracle's index, the profiles with brisk_amd.profile_from_slots
and the intervals with brisk_amd.intervals_from_profile of those.  Nothing expected is computed by the library under test.
tests/test_sharded_kmers_cpu.py shows from the oracle alone that the cases are not vacuous."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sharded_cases as C
import sharded_job as S
import sharded_kmers_job as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = 1


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    assert brisk_amd.library_path()
    return brisk_amd


# ---- the round trip ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", K.CUT_SCHEMES, ids=K.scheme_id)
@pytest.mark.parametrize("k,m,b", K.KMER_GEOMETRIES)
def test_round_trip(B, k, m, b, scheme):
    """2, 3 and 8 owners with equal ranges, with cut points balanced on the job's histogram and with cut points that leave a first,
    a middle and the last owner empty: every slot of present, absent, low-complexity, ragged, shorter-than-k and empty reads."""
    name, n_owners = scheme
    reads, queries = C.base_reads(), C.base_queries()
    K.check_case(B, reads, queries, k, m, b, n_owners, cuts=K.cuts_of(name, n_owners, reads, k, m, b))


@pytest.mark.parametrize("row", C.EDGE_ROWS, ids=C.row_id)
def test_boundary_geometries(B, row):
    K.check_case(B, C.edge_reads(row), C.edge_queries(row), row.k, row.m, row.b, 3, part_bits=row.part_bits)


@pytest.mark.parametrize("k,m,b", C.LONG_GEOMETRIES)
def test_long_sequences(B, k, m, b):
    """sequences of more than 8192 k-mers: the chunked scan, seams that are scanned again, a chunk's records placed by their sequence's slot base"""
    from test_kmer_query import assert_slots
    seqs, queries = C.long_sequences()
    want, alts, _ = K.expected(seqs, queries, k, m, b)
    with K.fill(B, seqs, k, m, b, 3) as job:
        assert_slots(K.round_trip(job, queries).slots, want, alts, (k, m, b, "long"))


@pytest.mark.parametrize("k,m,b", C.COUNT_GEOMETRIES)
def test_wrapped_and_saturating_counts(B, k, m, b):
    """a read inserted 256 times: 0x100 (present, count 0) in every slot under wrapping counts, 0x1ff under saturating ones"""
    from test_kmer_query import assert_slots
    reads, queries, hot = K.wrap_case(k)
    want, alts, base = K.expected(reads, queries, k, m, b)
    n_hot = int(base[1])
    assert n_hot == 21 and (want[:n_hot] == 0x100).all()
    for mode, value in ((None, 0x100), ("saturate", 0x1ff)):
        expect = want.copy()
        expect[:n_hot] = value
        with K.fill(B, reads, k, m, b, 3, count_mode=mode) as job:
            got = K.round_trip(job, queries).slots
        assert (got[:n_hot] == value).all(), (mode, got[:n_hot])
        assert_slots(got, expect, alts, (k, m, b, mode))


# ---- kernel variants, profiles and trimming: one process per environment -----------------------------------------------------------
def run_worker(name, args, env, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(HERE, name)] + args, env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1].startswith("ok "), (env, p.stdout[-2000:], p.stderr[-4000:])
    return p.stdout.strip().splitlines()[-1]


@pytest.mark.parametrize("env", C.VARIANT_ENVS, ids=lambda e: " ".join("%s=%s" % kv for kv in sorted(e.items())))
def test_kernel_variants_from_answer_records(B, env):
    """k_query<true> (BRISK_QUERY_GENERIC) and k_query_huge<true> (BRISK_HUGE_QUERY_AT) under answer_records' anchors: three owners,
    four geometries, a hot partition among the reads (tests/sharded_kmers_worker.py)"""
    assert run_worker("sharded_kmers_worker.py", ["variants"], env) == "ok %d" % len(C.VARIANT_GEOMETRIES)


@pytest.mark.parametrize("k,m,b", K.PROFILE_GEOMETRIES)
def test_profiles_and_rules_over_placed_slots(B, k, m, b):
    """profile_slots over the placed slots at solid_min 0, 2 and 300 against profile_from_slots of the oracle's slots; the solid_run
    and median rules over those records against intervals_from_profile"""
    K.check_case(B, C.base_reads(), C.base_queries(), k, m, b, 3, profiles=True)


def test_segmented_profiles(B):
    """BRISK_PROFILE_SEG=64: the 150 nt reads are reduced in segments and folded (the library reads the variable once per process)"""
    assert run_worker("sharded_kmers_worker.py", ["segments"], {"BRISK_PROFILE_SEG": "64"}) == "ok %d" % len(K.PROFILE_GEOMETRIES)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(B):
    import torch
    k, m, b = 31, 15, 14
    reads, queries = C.base_reads(), C.base_queries()[:80]
    with S.run(B, reads, k, m, b, 3) as job:
        ix = job.owners[0]
        L, h = ix.L, ix.h
        u64 = ctypes.c_uint64
        n_rec, n_slots = u64(), u64()
        assert L.brisk_hip_scan_kmers(h, None, None, 5, None, None, None, 0, ctypes.byref(n_rec), ctypes.byref(n_slots)) == EINVAL
        assert L.brisk_hip_scan_kmers(h, None, None, 0, None, None, None, 0, None, None) == EINVAL
        assert L.brisk_hip_scan_kmers(None, None, None, 0, None, None, None, 0, ctypes.byref(n_rec), ctypes.byref(n_slots)) == EINVAL
        assert L.brisk_hip_record_kmers(h, None, 5, None) == EINVAL and L.brisk_hip_record_kmers(None, None, 0, None) == EINVAL
        assert L.brisk_hip_answer_records(h, None, 5, None, None) == EINVAL and L.brisk_hip_answer_records(None, None, 0, None, None) == EINVAL
        assert L.brisk_hip_place_answers(h, None, None, None, 5, None, None, None, 10) == EINVAL
        assert L.brisk_hip_place_answers(None, None, None, None, 0, None, None, None, 0) == EINVAL
        assert L.brisk_hip_profile_slots(h, None, None, 5, 2, None) == EINVAL and L.brisk_hip_profile_slots(None, None, None, 0, 2, None) == EINVAL
        # the unsharded entry points stay closed on a sharded handle
        with pytest.raises(B.BriskHipError) as e:
            ix.get_kmers(queries)
        assert e.value.code == EINVAL and "sharded" in str(e.value)
        with pytest.raises(B.BriskHipError) as e:
            ix.read_profile(queries)
        assert e.value.code == EINVAL
        # place_answers with too few slots: EINVAL, nothing stored at or beyond n_slots, what was stored is right, the handle goes on
        t = K.round_trip(job, queries)
        small = t.n_slots // 2
        d_slots = torch.full((t.n_slots,), -1, dtype=torch.int16, device="cuda")
        args = (t.d_out.data_ptr(), t.d_tags_out.data_ptr(), t.d_anchors.data_ptr(), t.nq, t.d_offs.data_ptr(), t.d_answers.data_ptr(), d_slots.data_ptr())
        torch.cuda.synchronize()
        with pytest.raises(B.BriskHipError) as e:
            ix.place_answers(*args, small)
        assert e.value.code == EINVAL and "anchor" in str(e.value)
        got = d_slots.cpu().numpy().view(np.uint16)
        assert (got[small:] == K.FILL).all(), "a slot at or beyond n_slots was stored"
        placed = got[:small] != K.FILL
        assert placed.any() and np.array_equal(got[:small][placed], t.slots[:small][placed])
        ix.sync()
        ix.place_answers(*args, t.n_slots)  # all pieces in one call, into the same array
        assert np.array_equal(d_slots.cpu().numpy().view(np.uint16), t.slots)
        ix.sync()


# ---- ShardedCounter, four gloo ranks on one device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,b", C.RANKS_GEOMETRIES)
def test_sharded_counter_with_four_ranks(B, k, m, b):
    """exchange.ShardedCounter's get_kmers_packed, read_profile_packed in batches of 256 reads (rank 2 idles in the second),
    trim_packed, count_spectrum, prune(2, 255) and checksum, four processes on device 0 with unequal and empty shares
    (tests/sharded_kmers_ranks_worker.py), all against the oracle, which runs inside the worker on the CPU."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1", "--master-port",
                          str(31100 + os.getpid() % 300), os.path.join(HERE, "sharded_kmers_ranks_worker.py"), str(k), str(m), str(b)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert sorted(re.findall(r"ok rank (\d)", out.stdout)) == ["0", "1", "2", "3"], (out.stdout[-2000:], out.stderr[-4000:])
