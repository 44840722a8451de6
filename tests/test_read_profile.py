"""GPU: per-read abundance profiles (brisk_hip_read_profile_reads / _packed) against profile_from_slots -- the record's definition in
numpy -- over the slots brisk_hip_get_kmers gives for the same reads (get_kmers is pinned to the oracle by test_kmer_query.py), and,
for the fields that do not depend on the order of a read's slots, against the oracle's slots directly."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle
from read_profile_worker import (RUN_GEOMETRY, SOLID_MINS, assert_same, check_against_slots, expected_run, expected_solid, parity_reads,
                                 profile_packed, substitute)
from test_gpu_parity import SPECIAL, _random_reads
from test_kmer_query import GEOMETRIES, expected_all, oracle_index, query_set

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "read_profile_worker.py")
ORDER_FREE = ("n_kmers", "n_present", "n_solid", "min_present", "max_present", "median", "median_present", "sum")
EINVAL = 1


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    assert brisk_amd.library_path()
    return brisk_amd


@pytest.mark.parametrize("k,m,b", GEOMETRIES)
def test_profile_equals_the_reduction_of_the_slots(B, k, m, b):
    rng = random.Random(k * 100 + m + b)
    reads = parity_reads(rng)
    queries = query_set(rng, reads, k)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(reads)
        counts, found, base = check_against_slots(ix, queries, SOLID_MINS, (k, m, b))
    # the inputs exercise what they should: absent and present slots, counts of 1, 2 and more, reads without slots
    assert found.any() and not found.all()
    assert {1, 2}.issubset(set(np.unique(counts[found]).tolist())) and counts[found].max() > 3
    assert (np.diff(base.astype(np.int64)) == 0).any()


@pytest.mark.parametrize("k,m,b", [(63, 21, 14), (31, 11, 11)])
def test_order_free_fields_match_the_oracle(B, O, k, m, b):
    rng = random.Random(k + m + b)
    reads = parity_reads(rng)
    queries = query_set(rng, reads, k)
    h = oracle_index(O, reads, k, m, b)
    want_slots, _alts, base = expected_all(O, h, queries, k, m)  # (a palindromic vector's other ordering permutes a read's slots: these fields do not see it)
    O.index_free(h)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(reads)
        for s in (1, 2, 256):
            want = B.profile_from_slots((want_slots & 0xff).astype(np.uint8), (want_slots & 0x100) != 0, base, s)
            got = ix.read_profile(queries, s)
            for f in ORDER_FREE:
                assert np.array_equal(got[f], want[f]), (k, m, b, s, f)


def test_edges_of_the_wave_loop(B):
    """reads of 0 .. 193 slots around the multiples of 64, whole and with one substituted nucleotide that makes the absent stretch
    start or end exactly at slots 63, 64, 65, 127 and 128; two equal runs in one read.  (At RUN_GEOMETRY, where a stretch cut from an
    inserted read is all present: see expected_solid.)"""
    k, m, b = RUN_GEOMETRY
    rng = random.Random(64)
    genome = "".join(rng.choice("ACGT") for _ in range(600))
    cases = [(genome[:k - 1], [])]
    for i, n in enumerate((1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193)):
        q = genome[i:i + n + k - 1]
        cases.append((q, []))
        for x in (63, 64, 65, 127, 128):
            if x + k - 1 < len(q):
                cases.append((q, [x + k - 1]))  # absent from slot x on
            if x < len(q):
                cases.append((q, [x]))          # absent up to slot x
    x, y = (193 - k) // 2, (129 - k) // 2
    q = genome[5:5 + 193 + k - 1]
    cases.append((q, [x - 1 + k - 1]))          # [0, x - 1) and [x - 1 + k, 193): the second run is longer
    cases.append((q, [x + k - 1]))              # [0, x) and [x + k, 193): equal, the first wins
    q = genome[9:9 + 140 + k - 1]
    cases.append((q, [10, 10 + k + y - 3]))     # [11, 8 + y) and [8 + k + y, 140): the later one is longer
    cases.append((q, [10, 10 + k + y]))         # [11, 11 + y) and [11 + k + y, 140): equal
    queries = [substitute(q, subs) for q, subs in cases]
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads([genome, genome])
        _, found, base = check_against_slots(ix, queries, (0, 1, 2, 3), "edges")
        got = ix.read_profile(queries, 2)
    for i, (q, subs) in enumerate(cases):
        n = max(len(q) - k + 1, 0)
        assert got["n_kmers"][i] == n
        assert found[int(base[i]):int(base[i + 1])].tolist() == expected_solid(n, k, subs), ("the construction does not hold", i, subs)
        assert (int(got["run_start"][i]), int(got["run_len"][i])) == expected_run(n, k, subs), (i, n, subs, got[i])
        if not subs:
            assert got["n_solid"][i] == n and got["median"][i] == (2 if n else 0)
    assert expected_run(193, k, [x - 1 + k - 1]) == (x - 1 + k, x + 1) and expected_run(193, k, [x + k - 1]) == (0, x)
    assert expected_run(140, k, [10, 10 + k + y - 3]) == (8 + k + y, y + 3) and expected_run(140, k, [10, 10 + k + y]) == (11, y)


def test_a_wrapped_count_is_present_and_solid_only_at_zero(B):
    rng = random.Random(256)
    for k, m, b in ((63, 21, 14), (31, 11, 11)):
        r256 = "".join(rng.choice("ACGT") for _ in range(k))
        r255 = "".join(rng.choice("ACGT") for _ in range(k + 3))
        with B.BriskHip(k, m, b) as ix:
            ix.insert_reads([r256] * 256 + [r255] * 255)
            p1, p0 = ix.read_profile([r256, r255, "C" * k], 1), ix.read_profile([r256, r255, "C" * k], 0)
            check_against_slots(ix, [r256, r255, "C" * k], (0, 1, 255, 256), "wrap")
        assert (p1["n_kmers"][0], p1["n_present"][0], p1["n_solid"][0], p1["run_len"][0], p1["sum"][0]) == (1, 1, 0, 0, 0)
        assert (p0["n_present"][0], p0["n_solid"][0], p0["run_start"][0], p0["run_len"][0]) == (1, 1, 0, 1)
        assert (p1["n_kmers"][1], p1["n_present"][1], p1["n_solid"][1], p1["min_present"][1], p1["max_present"][1], p1["median"][1], p1["sum"][1]) == (4, 4, 4, 255, 255, 255, 1020)
        assert (p1["n_kmers"][2], p1["n_present"][2], p1["median"][2]) == (1, 0, 0)


def _run_worker(mode, extra):
    env = dict(os.environ, **extra)
    p = subprocess.run([sys.executable, WORKER, mode], env=env, capture_output=True, text=True, timeout=600)
    want = "ok 5" if mode == "segments" else "ok 4"
    assert p.returncode == 0 and p.stdout.strip().endswith(want), (extra, p.stdout[-2000:], p.stderr[-4000:])


@pytest.mark.parametrize("seg", ["64", "100"])
def test_segmented_path_with_a_small_threshold(B, seg):
    """BRISK_PROFILE_SEG is read once per process: a child each.  At 64 slots every 150 bp read of the parity case is segmented
    (88 slots at k = 63), at 100 those of the smaller k; the worker adds runs that begin and end at the boundaries +- 1 and one across three segments."""
    _run_worker("segments", {"BRISK_PROFILE_SEG": seg})


def test_long_sequences_with_the_default_threshold(B):
    """the sequences of test_long_sequences_are_answered_through_chunks: far above the default threshold"""
    rng = random.Random(2025)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    seqs = [rnd(60_017), rnd(8192 + 63), "A" * 30_000, "ACGTTGCA" * 4000, rnd(15_000) + "T" * 20_000 + rnd(15_000),
            rnd(5000) + "ACGTTGCA" * 3000 + rnd(5000) + rnd(64) * 200 + rnd(3000), rnd(2500) + "CA" * 9000 + rnd(2500)]
    seqs += _random_reads(rng, 200, 3000)
    queries = seqs + [rnd(20_000) + "A" * 90 + rnd(20_000), "A" * 70 + rnd(30_000)] + _random_reads(rng, 50, 3000)
    for k, m, b in ((63, 21, 14), (31, 11, 11)):
        with B.BriskHip(k, m, b) as ix:
            ix.insert_reads(seqs)
            _, found, _ = check_against_slots(ix, queries, (1, 2), ("long", k, m, b))
            assert not found.all()
            got = ix.read_profile(queries, 1)
        assert got["n_kmers"][0] == 60_017 - k + 1 == got["n_solid"][0] == got["run_len"][0]
        assert got["n_kmers"][2] == 30_000 - k + 1 == got["n_present"][2] == got["run_len"][2]  # (poly-A: several identities, so several counts)


def test_kernel_variants(B):
    """the probe bodies and record layouts of test_kernel_variants_match_the_oracle: the slots must reduce to the same records
    whichever kernels wrote them"""
    for extra in ({"BRISK_QUERY_GENERIC": "1"}, {"BRISK_BINS": "0"}, {"BRISK_BINS": "2", "BRISK_QUERY_ENT": "256"},
                  {"BRISK_HUGE_QUERY_AT": "0"}, {"BRISK_HUGE_QUERY_AT": "0", "BRISK_BINS": "2"}, {"BRISK_HUGE_QUERY_AT": "8", "BRISK_BINS": "0"}):
        _run_worker("parity", extra)


def test_batching_does_not_change_the_answer(B):
    rng = random.Random(11)
    reads = parity_reads(rng)
    queries = query_set(rng, reads, 63)
    outs = []
    for kw in ({}, {"max_batch_reads": 97}, {"max_batch_reads": 1}):
        with B.BriskHip(63, 21, 14, **kw) as ix:
            ix.insert_reads(reads)
            outs.append(ix.read_profile(queries, 2))
            if kw.get("max_batch_reads") == 97:
                assert_same(profile_packed(ix, queries, 2), outs[-1], "packed, batches of 97")
            if not kw:
                assert_same(outs[0], B.profile_from_slots(*ix.get_kmers(queries), 2), "default batches")
    assert_same(outs[1], outs[0], "batches of 97")
    assert_same(outs[2], outs[0], "batches of 1")


def test_deferred_inserts_are_completed_first(B):
    rng = random.Random(7)
    reads = _random_reads(rng, 500, 2000)
    with B.BriskHip(63, 21, 14) as ix:
        ix.insert_reads(reads[:250])
        ix.insert_reads(reads[250:])
        got = ix.read_profile(reads, 1)
    assert (got["n_kmers"] == 150 - 63 + 1).all()
    assert np.array_equal(got["n_present"], got["n_kmers"]) and np.array_equal(got["n_solid"], got["n_kmers"])
    assert (got["run_start"] == 0).all() and np.array_equal(got["run_len"], got["n_kmers"])


def test_refusals(B):
    import torch
    from test_kmer_query import packed_on_device
    reads = _random_reads(random.Random(5), 20, 500)
    for kw, word in ((dict(entry_ids=True), "entry-id"), (dict(n_owners=2, owner_rank=0), "sharded")):
        with B.BriskHip(31, 15, 14, **kw) as ix:
            with pytest.raises(B.BriskHipError) as e:
                ix.read_profile(reads)
            assert e.value.code == EINVAL and word in str(e.value) and "read_profile_reads" in str(e.value)
            d_packed, d_starts, _ = packed_on_device(ix, reads)
            d_out = torch.zeros(len(reads) * 32, dtype=torch.uint8, device="cuda")
            with pytest.raises(B.BriskHipError) as e:
                ix.read_profile_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), d_out.data_ptr())
            assert e.value.code == EINVAL and word in str(e.value) and "read_profile_packed" in str(e.value)
    with B.BriskHip(31, 15, 14) as ix:
        ix.insert_reads(reads)
        assert len(ix.read_profile([])) == 0
        assert ix.L.brisk_hip_read_profile_packed(ix.h, None, None, 0, 2, None) == 0
        flat, offs = oracle.pack_reads(reads)
        bad = offs.copy()
        bad[3], bad[4] = offs[4], offs[3]
        out = np.zeros(len(reads), B.READ_PROFILE_DTYPE)
        assert ix.L.brisk_hip_read_profile_reads(ix.h, flat, bad, len(reads), 2, out) == EINVAL
        assert b"ascend" in ix.L.brisk_hip_last_error(ix.h)
        d_packed, d_starts, _ = packed_on_device(ix, reads)
        d_bad = torch.from_numpy(bad.astype(np.int64)).cuda()
        d_out = torch.zeros(len(reads) * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(B.BriskHipError) as e:
            ix.read_profile_packed(d_packed.data_ptr(), d_bad.data_ptr(), len(reads), d_out.data_ptr())
        assert e.value.code == EINVAL and "ascend" in str(e.value)
        # the handle is as it was
        sums = ix.get_reads(reads)
        assert (sums > 0).all()
        got = ix.read_profile(reads, 1)
        assert np.array_equal(got["n_present"], got["n_kmers"])


def test_brisk_count_profile(B, tmp_path):
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe):
        B.build_apps()
    fasta = os.path.join(ROOT, "tests", "golden", "test.fa")
    seqs = oracle.fasta_sequences(open(fasta).read())
    k, m, b = 31, 11, 4
    names = ("n_kmers", "n_present", "n_solid", "run_start", "run_len", "min_present", "max_present", "median", "median_present", "sum")

    def run(extra):
        tsv = str(tmp_path / "profile.tsv")
        p = subprocess.run([exe, "--bulk", fasta, str(k), str(m), str(b), "--profile", tsv, "--solid", "2"] + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = open(tsv).read().splitlines()
        assert lines[0] == "#read_index\tn_kmers\tn_present\tn_solid\trun_start\trun_len\tmin\tmax\tmedian\tmedian_present\tsum"
        rows = [[int(x) for x in l.split("\t")] for l in lines[1:]]
        assert [r[0] for r in rows] == list(range(len(seqs))) and all(len(r) == 11 for r in rows)
        return rows

    rows = run([])
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(seqs)
        want = ix.read_profile(seqs, 2)
        for i, r in enumerate(rows):
            assert r[1:] == [int(want[f][i]) for f in names], (i, r, want[i])
        assert any(r[3] < r[2] for r in rows)  # k-mers seen once: present, not solid
        rows = run(["--min-count", "2"])       # they are pruned before the reads are profiled
        assert all(r[3] == r[2] for r in rows) and any(r[2] < r[1] for r in rows)
        ix.prune(2)
        want = ix.read_profile(seqs, 2)
        for i, r in enumerate(rows):
            assert r[1:] == [int(want[f][i]) for f in names], ("--min-count 2", i, r, want[i])
