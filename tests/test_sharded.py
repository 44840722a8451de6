"""The sharded count and get paths on one device against the oracle: N owners driven through the C-ABI by
tests/sharded_job.py, which asserts range, conservation, histogram, disjointness and checksums on the way; what the owners hold
together and what the get returns is compared here with Oracle.count, Oracle.index_query_reads and oracle.digest.  Nothing
expected is computed by the library under test.  tests/test_sharded_cpu.py shows from the oracle alone that the cases are not
vacuous."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sharded_cases as C
import sharded_job as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL, EUNSUPPORTED = 1, 2


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    assert brisk_amd.library_path()
    return brisk_amd


def count_and_get(B, reads, queries, k, m, b, n_owners, **kw):
    """one job: the owners together hold the oracle's index of `reads`, and the get across them is the oracle's query"""
    with S.run(B, reads, k, m, b, n_owners, **kw) as job:
        E = job.check()
        assert np.array_equal(S.get(B, job, queries), E.query(queries)), (k, m, b, n_owners, kw, "get")
        return job.records, job.layout, [s["nb_kmers"] for s in job.stats]


# ---- owner counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_owners", [2, 3, 5, 7, 8, "8 balanced"])
@pytest.mark.parametrize("k,m,b", C.COUNT_GEOMETRIES)
def test_owner_counts(B, k, m, b, n_owners):
    """2, 3, 5, 7 and 8 owners with equal ranges, and 8 with cut points balanced on the job's own histogram, at k63 m21 b14 and at
    (31, 11, 4), whose 23-bit routing id carries 14 hash bits and a class bit: count and get."""
    from brisk_amd import exchange as X
    reads, queries = C.base_reads(), C.base_queries()
    cuts = None
    if n_owners == "8 balanced":
        n_owners = 8
        d_hist, pb = S.job_histogram(B, reads, k, m, b)
        cuts = X.balanced_cuts(d_hist, pb, n_owners)
        assert cuts != X.uniform_cuts(pb, n_owners)
    count_and_get(B, reads, queries, k, m, b, n_owners, cuts=cuts)


# ---- boundary geometries -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", C.EDGE_ROWS, ids=C.row_id)
def test_boundary_geometries(B, row):
    """The key-layout boundary rows whose routing differs (tests/geometry_edges.py): three owners with equal ranges, then with cut
    points that fall on partitions holding records (taken from the first run's scanned records)."""
    boundary_geometry(B, row)


def boundary_geometry(B, row):
    k, m, b = row.k, row.m, row.b
    reads, queries = C.edge_reads(row), C.edge_queries(row)
    rec, lay, _ = count_and_get(B, reads, queries, k, m, b, 3, part_bits=row.part_bits)
    from geometry_edges import check_library_layout
    check_library_layout(row, dict(lay))
    part, n, _ = S.oracle_partitions(reads, k, m, b, row.part_bits)  # the scan's (partition, k-mers) per record are the oracle's
    assert S.same_rows(np.stack([S.partitions(rec, lay, b), S.instances(rec)], axis=1), np.stack([part, n], axis=1)), "routing ids"
    cuts = S.cuts_at_records(S.partitions(rec, lay, b), lay["part_bits"], 3)
    assert 0 < cuts[1] < cuts[2] < 1 << lay["part_bits"], cuts
    count_and_get(B, reads, queries, k, m, b, 3, part_bits=row.part_bits, cuts=cuts)


def test_eight_equal_owners_at_the_smallest_geometry(B):
    """(12, 5, 1): 2^11 partitions; eight equal owners are the 2-bit bucket id and the top bit of the minimizer's hash.  Every owner
    holds what the oracle's records say it holds (tests/test_sharded_cpu.py: uneven, none empty -- four would be empty if the
    owner came from the bucket id alone)."""
    row = C.SMALLEST
    reads, queries = C.edge_reads(row), C.edge_queries(row)
    rec, lay, entries = count_and_get(B, reads, queries, row.k, row.m, row.b, 8)
    part, n, _ = S.oracle_partitions(reads, row.k, row.m, row.b)
    assert S.same_rows(np.stack([S.partitions(rec, lay, row.b), S.instances(rec)], axis=1), np.stack([part, n], axis=1))
    from brisk_amd.exchange import uniform_cuts
    held = np.bincount(S.owner_of(part, uniform_cuts(lay["part_bits"], 8)), minlength=8)
    assert [e > 0 for e in entries] == [h > 0 for h in held.tolist()]


@pytest.mark.parametrize("row", C.EMPTY_OWNER_ROWS, ids=C.row_id)
def test_cut_points_with_empty_owners(B, row):
    """An empty first, middle and last owner, and one owner that holds everything (each of the three in turn)."""
    k, m, b = row.k, row.m, row.b
    reads, queries = C.edge_reads(row), C.edge_queries(row)
    lay = S.layout_of(k, m, b, row.part_bits)
    end = 1 << lay["part_bits"]
    c = C.middle_cut(row)
    for cuts in ([0, 0, c, end], [0, c, c, end], [0, c, end, end], [0, end, end, end], [0, 0, end, end], [0, 0, 0, end]):
        _, _, entries = count_and_get(B, reads, queries, k, m, b, 3, part_bits=row.part_bits, cuts=cuts)
        assert [e > 0 for e in entries] == [cuts[o + 1] > cuts[o] for o in range(3)], (cuts, entries)


def run_worker(name, args, env, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(HERE, name)] + args, env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1].startswith("ok "), (env, p.stdout[-2000:], p.stderr[-4000:])
    return p.stdout.strip().splitlines()[-1]


def test_three_class_bits(B):
    """BRISK_CLS_BITS=3 at (31, 11, 11): a 25-bit routing id, 2^25 partitions.  In a worker: the variable is read once per process."""
    assert run_worker("sharded_variant_worker.py", ["cls"], {"BRISK_CLS_BITS": "3"}) == "ok 4"


# ---- many owners -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,b", C.MANY_OWNER_GEOMETRIES)
def test_many_owners(B, O, k, m, b):
    """256 owners, the most the routing kernels take (their per-owner cursors live in LDS).  Routing needs one handle only: every
    record's owner is checked against numpy (sharded_job.scan_route: per-owner counts, every record inside its owner's range, the
    multiset kept) for equal ranges and for 256 random ascending cut points with repeats; then owners 0, 127 and 255 are created
    and filled, and each holds what the oracle says of its range."""
    import torch
    from brisk_amd.exchange import uniform_cuts
    N = 256
    reads = C.many_owner_reads(k, m, b)
    E = S.expect(reads, k, m, b)
    with B.BriskHip(k, m, b, owner_rank=0, n_owners=N) as ix:
        lay, W = ix.layout, ix.record_words
        pb = lay["part_bits"]
        d_packed, d_starts = S.to_device(ix, reads)
        d_acc = torch.zeros(1 << pb, dtype=torch.int64, device="cuda")
        equal = uniform_cuts(pb, N)
        d_out, counts, lens, rec = S.scan_route(ix, d_packed, d_starts, 0, len(reads), equal, b, d_acc, False, [])
        d_slices = d_acc.clone()
        part = S.partitions(rec, lay, b)
        for seed in (1, 2):
            cuts = C.random_cuts(seed, part, pb, N)
            ix.set_owner_cuts(cuts)
            _, c2, _, _ = S.scan_route(ix, d_packed, d_starts, 0, len(reads), cuts, b, d_acc, False, [])
            assert sum(1 for c in c2 if c) >= 8, "the random cut points leave fewer than eight owners with records"
    # what the oracle says an owner holds: its entries whose partition lies in the owner's range -- k63 m21 b14: a partition is a
    # bucket range, from Oracle.bucket_ids; with hash and class bits in the routing id: the oracle's enumerator stream
    # (identities) beside its records (routing ids), k-mer by k-mer.  There the k-mers of the oracle's records, counted per owner, must agree with that as well.
    if lay["ext_bits"] == 0:
        entry_part = O.bucket_ids(E.h, *E.dump[:3]).astype(np.int64) >> S.routing_shift(lay, b)
    else:
        from collections import Counter
        entry_part = S.entry_partitions(E, reads)
        _, kmers = S.oracle_pieces(reads, k, m, b, S.layout_of(k, m, b))
        per_owner = Counter(int(o) for o in S.owner_of(np.array([rid for rid, _, _ in Counter(kmers)], np.int64) >> S.routing_shift(lay, b), equal))
    owner_of_entry = S.owner_of(entry_part, equal)
    at = np.concatenate([[0], np.cumsum(counts)])
    for o in (0, 127, 255):
        with B.BriskHip(k, m, b, owner_rank=o, n_owners=N) as own:
            sl = d_slices[equal[o]:equal[o + 1]].clone()
            recv = d_out[int(at[o]) * W:int(at[o + 1]) * W].clone()
            torch.cuda.synchronize()
            own.insert_records_hist(recv.data_ptr() if counts[o] else 0, counts[o], sl.data_ptr(), 1)
            sel = owner_of_entry == o
            assert sel.any(), (k, m, b, o)
            assert np.array_equal(S.entry_rows(*own.enumerate()), S.entry_rows(*[a[sel] for a in E.dump])), (k, m, b, o)
            if lay["ext_bits"]:
                assert int(sel.sum()) == per_owner[o]


def test_refusals(B):
    """257 owners are refused at create; routing for more owners than there are partitions is refused with EINVAL and leaves
    the handle usable."""
    import torch
    with pytest.raises(B.BriskHipError) as e:
        B.BriskHip(63, 21, 14, owner_rank=0, n_owners=257)
    assert e.value.code == EUNSUPPORTED
    row = C.SIXTY_FOUR_PARTITIONS
    reads = C.edge_reads(row)[:60]
    with B.BriskHip(row.k, row.m, row.b, part_bits=row.part_bits, owner_rank=0, n_owners=65) as ix:
        assert 1 << ix.layout["part_bits"] == 64
        W = ix.record_words
        d_packed, d_starts = S.to_device(ix, reads)
        bound = ix.scan_bound(d_starts.data_ptr(), len(reads))
        d_rec = torch.zeros(bound * W, dtype=torch.int64, device="cuda")
        d_out = torch.zeros_like(d_rec)
        torch.cuda.synchronize()
        n_rec = ix.scan_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), d_rec.data_ptr(), bound)
        assert n_rec > 0
        with pytest.raises(B.BriskHipError) as e:
            ix.route_records(d_rec.data_ptr(), n_rec, d_out.data_ptr())
        assert e.value.code == EINVAL and "more owners than partitions" in str(e.value)
        assert ix.scan_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), d_rec.data_ptr(), bound) == n_rec
        d_hist = torch.zeros(64, dtype=torch.int64, device="cuda")
        ix.export_hist(d_hist.data_ptr())
        rec = S.host_rows(d_rec, n_rec, W)
        uniq, words = S.sparse_hist(S.partitions(rec, ix.layout, row.b), S.instances(rec))
        want = np.zeros(64, np.int64)
        want[uniq] = words
        assert np.array_equal(d_hist.cpu().numpy(), want)
        assert ix.stats()["nb_kmers"] == 0


# ---- long sequences ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,b", C.LONG_GEOMETRIES)
def test_long_sequences(B, k, m, b):
    """Sequences of more than 8192 k-mers are scanned as chunks; where a chunk's seam does not match the sequential state (long runs
    without a new minimum: the homopolymers and the tandem repeat here) the chunk is scanned again, the scan's histogram is thrown
    away and brisk_hip_scan_packed rebuilds it from the final records (k_part_hist).  That these inputs take the rebuild branch is
    read off the code (scan_impl: `out3.hist = nullptr` once a chunk is re-scanned, `hist_ok` false), not observed; the histogram
    invariant holds of whichever histogram is exported, partition by partition, and the slices travel into insert_records_hist.
    Three owners; the get of the same sequences and of three with poly-A stretches (where query_sequence stops) runs across them."""
    seqs, queries = C.long_sequences()
    with S.run(B, seqs, k, m, b, 3) as job:
        E = job.check(lines=False)
        assert sum(s["nb_kmers"] > 0 for s in job.stats) >= 2
        assert np.array_equal(S.get(B, job, queries), E.query(queries)), (k, m, b, "get")


# ---- pieces and modes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,b", C.COUNT_GEOMETRIES)
def test_three_pieces_with_summed_histograms(B, k, m, b):
    """every rank scans its share in three pieces; export_hist_add sums their histograms, one slice per owner travels"""
    count_and_get(B, C.base_reads(), C.base_queries()[:60], k, m, b, 3, pieces=3)


@pytest.mark.parametrize("k,m,b", C.COUNT_GEOMETRIES)
def test_owner_counts_for_itself(B, k, m, b):
    """insert_records: no histogram travels, the owner counts what it received"""
    count_and_get(B, C.base_reads(), C.base_queries()[:60], k, m, b, 3, with_hist=False)


def test_second_batch_meets_existing_entries(B):
    reads, queries = C.base_reads(), C.base_queries()
    half = len(reads) // 2
    for k, m, b in C.COUNT_GEOMETRIES:
        job = S.run(B, reads[:half], k, m, b, 3)
        with S.run(B, reads[half:], k, m, b, 3, job=job, pieces=2):
            E = job.check()
            assert np.array_equal(S.get(B, job, queries), E.query(queries))


def test_foreign_records_and_wrong_slices_are_refused(B):
    """insert_records refuses records of another owner, insert_records_hist slices whose record total is not the number of records
    handed over; nothing is inserted and the handle takes the right call afterwards."""
    import torch
    reads = C.base_reads()
    for k, m, b in C.COUNT_GEOMETRIES:
        with S.Job(B, k, m, b, 3, None, 0, None) as job:
            W = job.owners[0].record_words
            inbox, slices = S.scan_all(job, reads)
            n = [t.numel() // W for t in inbox]
            assert min(n) > 1
            torch.cuda.synchronize()
            with pytest.raises(B.BriskHipError) as e:
                job.owners[0].insert_records(inbox[1].data_ptr(), n[1])
            assert e.value.code == EINVAL and "other owners" in str(e.value)
            mixed = torch.cat([inbox[0][W:], inbox[2][:W]])  # one foreign record among the owner's own
            torch.cuda.synchronize()
            with pytest.raises(B.BriskHipError) as e:
                job.owners[0].insert_records(mixed.data_ptr(), n[0])
            assert e.value.code == EINVAL and "1 records belong to other owners" in str(e.value)
            with pytest.raises(B.BriskHipError) as e:
                job.owners[1].insert_records_hist(inbox[1].data_ptr(), n[1] - 1, slices[1].data_ptr(), 3)
            assert e.value.code == EINVAL and "slices count" in str(e.value)
            with pytest.raises(B.BriskHipError) as e:  # two of the three slices: fewer records than were handed over
                job.owners[1].insert_records_hist(inbox[1].data_ptr(), n[1], slices[1].data_ptr(), 2)
            assert e.value.code == EINVAL and "slices count" in str(e.value)
            assert [ix.stats()["nb_kmers"] for ix in job.owners] == [0, 0, 0]
            job.owners[0].insert_records(inbox[0].data_ptr(), n[0])
            job.owners[1].insert_records_hist(inbox[1].data_ptr(), n[1], slices[1].data_ptr(), 3)
            job.owners[2].insert_records_hist(inbox[2].data_ptr(), n[2], slices[2].data_ptr(), 3)
            job.reads = list(reads)
            job.collect()
            job.check()


def test_owner_batch_goes_in_halves_when_the_arena_reserve_does_not_fit(B, monkeypatch):
    """BRISK_ARENA_LIMIT as test_batch_splits_when_the_arena_reserve_does_not_fit sets it, sized for the owner's share: the
    insert_records_hist batch does not fit "every instance is new", goes in as halves (which the owner counts itself), and the
    index is the same.  As in that test, that the batch went in halves is not observed (the library reports nothing about it): it
    follows from the limit, which assumes that an owner's share under equal ranges at k63 is about a third (DESIGN.md section 5:
    max / mean 1.01) and that the reserve is the instances with a quarter of headroom (grow_cap) -- 0.42 of the job's instances
    against a limit of 0.33, and 0.21 for a half.  The second setting shows that the limit reaches this path at all."""
    k, m, b = 63, 21, 14
    reads = C.base_reads()
    monkeypatch.delenv("BRISK_NO_VMM", raising=False)
    with B.BriskHip(k, m, b) as probe:
        slack = probe.insert_slack()
    assert slack > 0
    inst = sum(max(0, len(r) - k + 1) for r in reads)
    monkeypatch.setenv("BRISK_ARENA_LIMIT", str(slack + inst // 3))  # an owner's third of the instances (reserved with a quarter of headroom) does not fit, a sixth does
    count_and_get(B, reads, C.base_queries()[:40], k, m, b, 3)
    monkeypatch.setenv("BRISK_ARENA_LIMIT", "1000")  # nothing fits: a clean error from the owner
    with pytest.raises(B.BriskHipError) as e:
        S.run(B, reads, k, m, b, 3)
    assert e.value.code == 4


def test_saturating_owners(B):
    """count_mode="saturate" on every owner (exchanged records carry no multiplicity): reads whose counts stay far below 255, so
    the oracle's wrapping counts are the expectation"""
    reads = C.saturate_reads()
    for k, m, b in C.COUNT_GEOMETRIES:
        with S.run(B, reads, k, m, b, 3, count_mode="saturate") as job:
            assert all(ix.count_mode == "saturate" for ix in job.owners)
            E = job.check()
            assert np.array_equal(S.get(B, job, C.base_queries()[:60]), E.query(C.base_queries()[:60]))


# ---- kernel variants ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", C.VARIANT_ENVS, ids=lambda e: " ".join("%s=%s" % kv for kv in sorted(e.items())))
def test_kernel_variants_from_the_sharded_entry_points(B, env):
    """The run-time-geometry insert / query bodies and the workgroup-per-partition kernels, which a sharded handle (classic record
    layout, no deferral) never reaches by itself: count and get on three owners at four geometries, a hot partition among the
    reads.  One process per environment (tests/sharded_variant_worker.py)."""
    assert run_worker("sharded_variant_worker.py", ["variants"], env) == "ok 8"


# ---- ShardedCounter, four gloo ranks on one device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,b", C.RANKS_GEOMETRIES)
def test_sharded_counter_with_four_ranks(B, k, m, b):
    """exchange.ShardedCounter as a job uses it, four processes on device 0 (tests/sharded_ranks_worker.py): balance() -- cut points
    at k31 m15 b14, none at (31, 11, 4) --, two count_packed batches with unequal and empty shares, the first of which outgrows the
    six-records-a-read estimate and goes through the regrowth, stats, summed checksums and get_packed of present and absent reads,
    all against the oracle, which runs inside the worker on the CPU."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1", "--master-port",
                          str(30700 + os.getpid() % 300), os.path.join(HERE, "sharded_ranks_worker.py"), str(k), str(m), str(b)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    import re
    assert sorted(re.findall(r"ok rank (\d)", out.stdout)) == ["0", "1", "2", "3"], (out.stdout[-2000:], out.stderr[-4000:])
