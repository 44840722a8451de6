"""GPU: count spectrum, count-range enumeration and prune against the CPU oracle, bit-exact.

Expected values always come from the oracle's index_dump of the same reads, binned or filtered with numpy, Oracle.digest_entries
for checksums and Oracle.bucket_ids for bucket counts -- never from the library under test (where a test also compares the
library with itself -- the order of the survivors, the slots before and after a prune -- it says so).  All three entry points
compare the stored count byte (counts are kept mod 256).

Geometries: k63 m21 b14 (two-word keys), k31 m15 b14 (one-word keys), k31 m11 b11 (a class bit in the routing id, big
partitions), k47 m13 b8 with the default partitions (ext_bits = 8: a partition is a slice of one bucket) and with part_bits
given (plain bucket ranges, 16 buckets a partition), and k63 m21 b14 with part_bits = 20 (256 buckets a partition: the bitmap
of brisk_hip_stats' own rebuild)."""
import ctypes as C
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle
from test_gpu_parity import SPECIAL, _random_reads

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY = 1, 5
GEOMS = [((63, 21, 14), {}), ((31, 15, 14), {}), ((31, 11, 11), {}), ((47, 13, 8), {}), ((47, 13, 8), dict(part_bits=12)), ((63, 21, 14), dict(part_bits=20))]
GEOM_IDS = ["k63m21b14", "k31m15b14", "k31m11b11", "k47m13b8-ext", "k47m13b8-pb12", "k63m21b14-pb20"]
RANGES = [(1, 1), (2, 255), (0, 0), (0, 255), (3, 9)]


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


def mixed_reads(seed, n=600, glen=5000):
    """coverage 18 with a part of the reads repeated (counts from 1 to a few dozen), the low-complexity set, ragged reads"""
    rng = random.Random(seed)
    base = _random_reads(rng, n, glen)
    reads = base + base[:200] * 2 + base[:40] * 5 + SPECIAL
    reads += ["".join(rng.choice("ACGT") for _ in range(rng.randint(1, 400))) for _ in range(40)]
    return reads


def oracle_index(O, reads, k, m, b):
    h = O.index_new(k, m, b)
    flat, offs = oracle.pack_reads(reads)
    O.index_insert_reads(h, flat, offs)
    return h


def keep(dump, lo, hi):
    mask = (dump[3] >= lo) & (dump[3] <= hi)
    return tuple(a[mask] for a in dump)


def entries(dump):
    """sorted (hi, lo, idx, cnt) rows: the multiset as one array"""
    rows = np.zeros(len(dump[0]), dtype=[("hi", np.uint64), ("lo", np.uint64), ("idx", np.uint8), ("cnt", np.uint8)])
    rows["lo"], rows["hi"], rows["idx"], rows["cnt"] = dump
    return np.sort(rows, order=["hi", "lo", "idx", "cnt"])


def same_multiset(got, want):
    return len(got[0]) == len(want[0]) and np.array_equal(entries(got), entries(want))


def want_stats(O, h, dump):
    """nb_kmers, nb_buckets of the index holding exactly `dump`"""
    return len(dump[0]), len(np.unique(O.bucket_ids(h, dump[0], dump[1], dump[2])))


def partition_of(O, h, dump, lay):
    """partition of every entry, from the oracle's bucket ids and the layout: partition = routing id >> shift, routing id = bucket
    id, then ext_bits - cls_bits more hash bits (not known here: usable when there are none), then the class of minimizer_idx"""
    assert lay["ext_bits"] == lay["cls_bits"]
    ids = O.bucket_ids(h, dump[0], dump[1], dump[2]).astype(np.int64)
    if lay["cls_bits"]:
        cls = np.minimum(dump[2].astype(np.int64) // lay["cls_width"], (1 << lay["cls_bits"]) - 1)
        ids = (ids << lay["cls_bits"]) | cls
    return ids >> (2 * lay["b"] + lay["ext_bits"] - lay["part_bits"])


def largest_partition(O, h, dump, lay):
    return int(np.unique(partition_of(O, h, dump, lay), return_counts=True)[1].max()) if len(dump[0]) else 0


def refused_somewhere(ix, cap, lo, hi):
    """walks brisk_hip_enumerate_range with `cap`: True when a call is refused with ECAPACITY (passing entries of one partition > cap)"""
    cursor = 0
    while True:
        rc, part, cursor = raw_range(ix, cap, lo, hi, cursor)
        if rc == ECAPACITY:
            return True
        assert rc == 0
        if len(part[0]) == 0:
            return False


def check_spectrum(ix, dump):
    got = ix.count_spectrum()
    assert got.dtype == np.uint64 and got.shape == (256,)
    assert np.array_equal(got, np.bincount(dump[3], minlength=256).astype(np.uint64))
    assert int(got.sum()) == ix.stats()["nb_kmers"] == len(dump[3])
    assert int((got * np.arange(256, dtype=np.uint64)).sum()) == ix.checksum()[1] == int(dump[3].astype(np.int64).sum())
    return got


def raw_range(ix, cap, lo, hi, cursor=0):
    """one brisk_hip_enumerate_range call -> (status, entries, cursor after)"""
    cur, n = C.c_uint64(cursor), C.c_uint64(0)
    a, b_, c, d = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
    rc = ix.L.brisk_hip_enumerate_range(ix.h, C.byref(cur), a, b_, c, d, cap, C.byref(n), lo, hi)
    return rc, tuple(x[:n.value].copy() for x in (a, b_, c, d)), cur.value


def walk_range(ix, cap, lo, hi):
    out, cursor, steps = [], 0, 0
    while True:
        rc, part, cursor = raw_range(ix, cap, lo, hi, cursor)
        assert rc == 0, (rc, cap, lo, hi)
        if len(part[0]) == 0:
            break
        out.append(part)
        steps += 1
    cat = tuple(np.concatenate([p[i] for p in out]) if out else np.zeros(0, dt) for i, dt in enumerate((np.uint64, np.uint64, np.uint8, np.uint8)))
    return cat, steps


# ---- 1: spectrum ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts", GEOMS, ids=GEOM_IDS)
def test_spectrum_equals_the_oracles_bincount(B, O, kmb, opts):
    k, m, b = kmb
    reads = mixed_reads(k * 100 + m)
    h = oracle_index(O, reads, k, m, b)
    dump = O.index_dump(h)
    assert len(np.unique(dump[3])) > 5  # mixed counts: the case is not one bin
    with B.BriskHip(k, m, b, **opts) as ix:
        ix.insert_reads(reads)
        if kmb == (47, 13, 8):
            assert (ix.layout["ext_bits"] > 0) == (not opts)
        check_spectrum(ix, dump)
    O.index_free(h)


def test_spectrum_of_counts_that_wrap(B, O):
    s = "ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGGCTAGCTAGCTAGGCTAGCCATAGACCAGATTTACAGGATACCCAGGGTAAACCA"
    rng = random.Random(3)
    reads = [s] * 256 + _random_reads(rng, 100, 2000) + ["ACGT" * 40] * 3
    for k, m, b in ((63, 21, 14), (31, 15, 14)):
        h = oracle_index(O, reads, k, m, b)
        dump = O.index_dump(h)
        with B.BriskHip(k, m, b) as ix:
            for i in range(0, len(reads), 100):
                ix.insert_reads(reads[i:i + 100])
            got = check_spectrum(ix, dump)
            assert got[0] > 0  # 256 inserts of one read: its k-mers are present with a stored count of 0
            # and they are entries like any other for a range and for prune
            assert same_multiset(ix.enumerate(min_count=0, max_count=0), keep(dump, 0, 0))
            assert ix.prune(1, 255) == int(got[0])
            assert ix.count_spectrum()[0] == 0 and ix.checksum() == O.digest_entries(*keep(dump, 1, 255))
        O.index_free(h)


def test_spectrum_of_an_empty_index_and_with_deferred_inserts_pending(B, O):
    k, m, b = 63, 21, 14
    reads = mixed_reads(77, n=300)
    h = oracle_index(O, reads, k, m, b)
    dump = O.index_dump(h)
    with B.BriskHip(k, m, b) as ix:  # default options: these small batches are deferred
        assert not ix.count_spectrum().any()
        assert ix.prune(2) == 0 and len(ix.enumerate(min_count=1, max_count=1)[0]) == 0
        for i in range(0, len(reads), 50):
            ix.insert_reads(reads[i:i + 50])
        assert np.array_equal(ix.count_spectrum(), np.bincount(dump[3], minlength=256).astype(np.uint64))
        ix.insert_reads(reads[:50])
        h2 = oracle_index(O, reads + reads[:50], k, m, b)
        d2 = O.index_dump(h2)
        assert same_multiset(ix.enumerate(min_count=2, max_count=255), keep(d2, 2, 255))  # the range walk completes them too
        ix.insert_reads(reads[:50])
        h3 = oracle_index(O, reads + reads[:50] * 2, k, m, b)
        d3 = O.index_dump(h3)
        assert ix.prune(2, 255) == len(keep(d3, 0, 1)[0])  # and so does prune
        assert ix.checksum() == O.digest_entries(*keep(d3, 2, 255))
        for x in (h2, h3):
            O.index_free(x)
    O.index_free(h)


# ---- 2: enumerate range -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts", GEOMS[:4], ids=GEOM_IDS[:4])
def test_enumerate_range(B, O, kmb, opts):
    k, m, b = kmb
    reads = mixed_reads(k * 100 + m + 1)
    h = oracle_index(O, reads, k, m, b)
    dump = O.index_dump(h)
    with B.BriskHip(k, m, b, **opts) as ix:
        ix.insert_reads(reads)
        for lo, hi in RANGES:
            assert same_multiset(ix.enumerate(min_count=lo, max_count=hi), keep(dump, lo, hi)), (lo, hi)
        rc, _, _ = raw_range(ix, 1 << 16, 7, 3)
        assert rc == EINVAL
        # [0, 255] through the range entry point: brisk_hip_enumerate's output entry for entry, in order
        plain = ix.enumerate()
        whole, _ = walk_range(ix, 1 << 20, 0, 255)
        assert all(np.array_equal(x, y) for x, y in zip(whole, plain))
        # many cursor steps give the sequence of one large call (a cap of the largest partition is never refused)
        one, steps1 = walk_range(ix, 1 << 20, 2, 255)
        many, steps = walk_range(ix, ix.stats()["largest_bucket"], 2, 255)
        assert steps1 == 1 and steps >= 10 and all(np.array_equal(x, y) for x, y in zip(many, one))
        mask = (plain[3] >= 2)
        assert all(np.array_equal(x, y[mask]) for x, y in zip(one, plain))  # storage order (the library's own, before the filter)
    O.index_free(h)


def test_enumerate_range_capacity_is_about_passing_entries(B, O):
    """four partitions of many entries of which few pass: a cap below one partition's passing entries is refused, a cap below
    every partition's size but not below any partition's passing entries is not"""
    k, m, b = 31, 11, 4
    rng = random.Random(9)
    reads = _random_reads(rng, 400, 3000)
    reads = reads + reads[:20]
    h = oracle_index(O, reads, k, m, b)
    dump = O.index_dump(h)
    with B.BriskHip(k, m, b, part_bits=2) as ix:
        ix.insert_reads(reads)
        assert ix.layout["ext_bits"] == 0 and ix.layout["part_bits"] == 2
        part = partition_of(O, h, dump, ix.layout)
        total = np.bincount(part, minlength=4)
        vals, freq = np.unique(dump[3], return_counts=True)
        v = int(vals[np.argmin(freq)])  # the rarest count
        passing = np.bincount(part[dump[3] == v], minlength=4)
        assert 0 < passing.max() < total[total > 0].min()
        assert refused_somewhere(ix, int(passing.max()) - 1, v, v)
        got, _ = walk_range(ix, int(passing.max()), v, v)
        assert same_multiset(got, keep(dump, v, v))
        assert refused_somewhere(ix, int(passing.max()), 0, 255)  # the same cap does not hold a whole partition
    O.index_free(h)


# ---- 3: prune -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts", GEOMS, ids=GEOM_IDS)
def test_prune_leaves_the_index_of_the_remaining_entries(B, O, kmb, opts):
    k, m, b = kmb
    reads = mixed_reads(k * 100 + m + 2)
    h = oracle_index(O, reads, k, m, b)
    dump = O.index_dump(h)
    for lo, hi in ((2, 255), (1, 1), (3, 9), (0, 0)):
        left = keep(dump, lo, hi)
        with B.BriskHip(k, m, b, **opts) as ix:
            ix.insert_reads(reads)
            before = ix.enumerate()
            skm = ix.stats()["nb_skmers"]
            assert ix.prune(lo, hi) == len(dump[0]) - len(left[0])
            st = ix.stats()
            assert (st["nb_kmers"], st["nb_buckets"]) == want_stats(O, h, left), (lo, hi)
            assert st["nb_skmers"] == skm
            if ix.layout["ext_bits"] == ix.layout["cls_bits"]:
                assert st["largest_bucket"] == largest_partition(O, h, left, ix.layout)
            assert ix.checksum() == O.digest_entries(*left)
            after = ix.enumerate()
            assert same_multiset(after, left)
            mask = (before[3] >= lo) & (before[3] <= hi)
            assert all(np.array_equal(x, y[mask]) for x, y in zip(after, before))  # the survivors keep their order
            assert np.array_equal(ix.count_spectrum(), np.bincount(left[3], minlength=256).astype(np.uint64))
    O.index_free(h)


def test_prune_corner_cases(B, O):
    k, m, b = 63, 21, 14
    reads = mixed_reads(5)
    h = oracle_index(O, reads, k, m, b)
    dump = O.index_dump(h)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(reads)
        cs = ix.checksum()
        assert cs == O.digest_entries(*dump)
        assert ix.prune(0, 255) == 0 and ix.checksum() == cs
        assert ix.prune(0) == 0 and ix.checksum() == cs  # max_count defaults to 255
        ones = keep(dump, 1, 1)
        assert ix.prune(1, 1) == len(dump[0]) - len(ones[0])
        assert ix.prune(1, 1) == 0  # nothing is left to remove
        assert ix.checksum() == O.digest_entries(*ones)
        assert ix.prune(200, 255) == len(ones[0])  # everything goes
        st = ix.stats()
        assert (st["nb_kmers"], st["nb_buckets"], st["largest_bucket"]) == (0, 0, 0)
        assert ix.checksum() == (0, 0, 0) and len(ix.enumerate()[0]) == 0 and not ix.count_spectrum().any()
        # and the empty index takes reads again as a new one does
        ix.insert_reads(reads)
        assert ix.checksum() == cs
    O.index_free(h)


# ---- 4: prune, then use ---------------------------------------------------------------------------------------------------------
def merged(first, second):
    """entries of `first` and `second` added up: counts mod 256 per (kmer, minimizer_idx)"""
    acc = {}
    for d in (first, second):
        for l, h_, i, c in zip(*(x.tolist() for x in d)):
            acc[(h_, l, i)] = (acc.get((h_, l, i), 0) + c) & 0xff
    keys = list(acc)
    return (np.array([x[1] for x in keys], np.uint64), np.array([x[0] for x in keys], np.uint64), np.array([x[2] for x in keys], np.uint8),
            np.array([acc[x] for x in keys], np.uint8))


@pytest.mark.parametrize("kmb,opts", GEOMS[:4], ids=GEOM_IDS[:4])
def test_gets_lookups_and_inserts_after_a_prune(B, O, kmb, opts):
    from test_kmer_query import assert_slots, expected_all
    k, m, b = kmb
    lo, hi = 2, 12
    rng = random.Random(k + m)
    reads = mixed_reads(k * 100 + m + 3)
    h = oracle_index(O, reads, k, m, b)
    dump = O.index_dump(h)
    left, gone = keep(dump, lo, hi), tuple(a[(dump[3] < lo) | (dump[3] > hi)] for a in dump)
    assert len(left[0]) and len(gone[0])
    queries = reads[:150] + _random_reads(rng, 30, 3000)
    with B.BriskHip(k, m, b, **opts) as ix:
        ix.insert_reads(reads)
        c0, f0, base = ix.get_kmers(queries)
        sums0 = ix.get_reads(queries)
        assert ix.prune(lo, hi) == len(gone[0])
        c1, f1, base1 = ix.get_kmers(queries)
        # the slots before the prune, those of the removed entries set to absent (the library against itself, as a caller sees it)
        stay = f0 & (c0 >= lo) & (c0 <= hi)
        assert np.array_equal(f1, stay) and np.array_equal(c1[stay], c0[stay]) and not c1[~stay].any()
        # and against the oracle: its per-slot answers with the removed entries' slots absent
        want, alts, wbase = expected_all(O, h, [q.upper() for q in queries], k, m)
        wcnt = (want & 0xff).astype(np.int64)
        want_after = np.where(((want & 0x100) != 0) & (wcnt >= lo) & (wcnt <= hi), want, 0).astype(np.uint16)
        alts_after = [(s, e, np.where(((v & 0x100) != 0) & ((v & 0xff) >= lo) & ((v & 0xff) <= hi), v, 0).astype(np.uint16)) for s, e, v in alts]
        got = np.where(f1, 0x100 | c1.astype(np.uint16), 0).astype(np.uint16)
        assert_slots(got, want_after, alts_after, (kmb, "get_kmers after prune"))
        # per-read sums: where a read's sum was the sum of its slots before (no stop at a zero minimizer), it is so after
        seg = lambda v: np.array([int(v[int(base[r]):int(base[r + 1])].astype(np.int64).sum()) for r in range(len(queries))], np.uint64)
        plain = seg(np.where(f0, c0, 0)) == sums0
        assert plain.mean() > 0.9
        sums1 = ix.get_reads(queries)
        assert np.array_equal(sums1[plain], seg(np.where(f1, c1, 0))[plain])
        # lookups: none of the removed pairs, all of the others with their counts
        data, found = ix.lookup(gone[0], gone[1], gone[2])
        assert not found.any()
        data, found = ix.lookup(left[0], left[1], left[2])
        assert found.all() and np.array_equal(data, left[3])
        # a second batch: new reads and reads of batch 1, whose removed k-mers come back with batch 2's count alone
        batch2 = reads[100:400] + _random_reads(rng, 200, 4000)
        h2 = oracle_index(O, batch2, k, m, b)
        d2 = O.index_dump(h2)
        g = set(zip(gone[1].tolist(), gone[0].tolist(), gone[2].tolist()))
        assert sum((x in g) for x in zip(d2[1].tolist(), d2[0].tolist(), d2[2].tolist())) > 100  # batch 2 does re-insert removed k-mers
        ix.insert_reads(batch2)
        want2 = merged(left, d2)
        assert same_multiset(ix.enumerate(), want2)
        st = ix.stats()
        assert (st["nb_kmers"], st["nb_buckets"]) == want_stats(O, h, want2)
        assert ix.checksum() == O.digest_entries(*want2)
        O.index_free(h2)
    O.index_free(h)


# ---- 5: a partition of many chunks, and a hot one ---------------------------------------------------------------------------------
def hot_partition_reads(O, k, m, seed):
    """Reads built round ONE minimizer (the m-mer with the smallest order key of 40 000 candidates, so that no other m-mer of
    a read beats it): random flanks, so every read adds k - m + 1 distinct k-mers to that minimizer's partitions; parts of the
    set are repeated (mixed counts).  With them: tandem reads and a homopolymer run many times (one hot, small partition) and
    ordinary reads."""
    rng = random.Random(seed)
    cands = [rng.randrange(1 << (2 * m)) for _ in range(40000)]
    best = cands[int(np.argmin(O.key_many(cands, m)))]
    mini = "".join("ACTG"[(best >> (2 * (m - 1 - i))) & 3] for i in range(m))
    flank = k - m
    hot = ["".join(rng.choice("ACGT") for _ in range(flank)) + mini + "".join(rng.choice("ACGT") for _ in range(flank)) for _ in range(900)]
    reads = hot + hot[:300] + hot[:100] * 5 + hot[:20] * 30
    reads += ["ACG" * 50] * 40 + ["A" * 150] * 300 + ["ACGTTGCA" * 18] * 7
    reads += _random_reads(rng, 300, 4000)
    return reads


def test_big_and_hot_partitions(B, O):
    k, m, b = 31, 11, 11
    reads = hot_partition_reads(O, k, m, 17)
    h = oracle_index(O, reads, k, m, b)
    dump = O.index_dump(h)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(reads)
        part = partition_of(O, h, dump, ix.layout)
        ids, sizes = np.unique(part, return_counts=True)
        big = int(ids[np.argmax(sizes)])
        assert sizes.max() > 4096, int(sizes.max())  # more than 64 chunks of 64 entries in one partition
        assert ix.stats()["largest_bucket"] == int(sizes.max())
        assert refused_somewhere(ix, 4096, 0, 255)  # and seen from the enumeration: 4096 entries do not hold every partition
        check_spectrum(ix, dump)
        for lo, hi in RANGES:
            assert same_multiset(ix.enumerate(min_count=lo, max_count=hi), keep(dump, lo, hi)), (lo, hi)
        before = ix.enumerate()
        lo, hi = 2, 6
        left = keep(dump, lo, hi)
        left_big = int((partition_of(O, h, left, ix.layout) == big).sum())
        assert 64 < left_big < sizes.max()  # the big partition loses entries and keeps several chunks of them
        assert ix.prune(lo, hi) == len(dump[0]) - len(left[0])
        st = ix.stats()
        assert (st["nb_kmers"], st["nb_buckets"]) == want_stats(O, h, left) and st["largest_bucket"] == largest_partition(O, h, left, ix.layout)
        assert ix.checksum() == O.digest_entries(*left)
        after = ix.enumerate()
        mask = (before[3] >= lo) & (before[3] <= hi)
        assert same_multiset(after, left) and all(np.array_equal(x, y[mask]) for x, y in zip(after, before))
        # the pruned index takes the reads again: survivors add up, removed k-mers start over
        ix.insert_reads(reads)
        want2 = merged(left, dump)
        assert ix.checksum() == O.digest_entries(*want2) and same_multiset(ix.enumerate(), want2)
    O.index_free(h)


# ---- 6: working density ---------------------------------------------------------------------------------------------------------
def test_working_density_case_b():
    """case B of tests/density_parity_worker.py (400 k error-bearing reads, k63 m21 b14) in a child process under its own time
    limit: tests/spectrum_density_worker.py"""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "spectrum_density_worker.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("BRISK_") or k == "BRISK_HIP_LIB"}
    t0 = time.time()
    p = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=900)
    print(f"density case B: {time.time() - t0:.0f} s")
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout[-6000:], p.stderr[-6000:])


# ---- 7: sharded handle ------------------------------------------------------------------------------------------------------------
def test_two_owners_spectra_and_pruned_digests_add_up(B, O):
    import torch
    rng = random.Random(41)
    reads = _random_reads(rng, 800, 6000) + SPECIAL
    reads = reads + reads[:300]
    for k, m, b in ((63, 21, 14), (31, 11, 4)):
        h = oracle_index(O, reads, k, m, b)
        dump = O.index_dump(h)
        flat, offs = oracle.pack_reads(reads)
        owners = [B.BriskHip(k, m, b, owner_rank=r, n_owners=2) for r in range(2)]
        d_bases = torch.from_numpy(flat).cuda()
        d_packed = torch.zeros((len(flat) + 15) // 16 + 4, dtype=torch.int32, device="cuda")
        d_starts = torch.from_numpy(offs.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        ix0 = owners[0]
        ix0.pack_ascii(d_bases.data_ptr(), len(flat), d_packed.data_ptr())
        ix0.sync()
        W = ix0.record_words
        half = len(reads) // 2
        inbox = [[], []]
        for r, (a, z) in enumerate(((0, half), (half, len(reads)))):  # each "rank" scans half of the reads
            ix = owners[r]
            st = d_starts[a:z + 1].contiguous()
            bound = ix.scan_bound(st.data_ptr(), z - a)
            d_rec = torch.zeros(max(bound, 1) * W, dtype=torch.int64, device="cuda")
            d_out = torch.zeros_like(d_rec)
            torch.cuda.synchronize()
            n_rec = ix.scan_packed(d_packed.data_ptr(), st.data_ptr(), z - a, d_rec.data_ptr(), bound)
            counts = ix.route_records(d_rec.data_ptr(), n_rec, d_out.data_ptr())
            ix.sync()
            o0 = int(counts[0])
            inbox[0].append(d_out[: o0 * W].clone())
            inbox[1].append(d_out[o0 * W: n_rec * W].clone())
        spectra, digests, removed, held = [], [], 0, []
        for r in range(2):
            recv = torch.cat(inbox[r])
            torch.cuda.synchronize()
            owners[r].insert_records(recv.data_ptr(), recv.numel() // W)
            spectra.append(owners[r].count_spectrum())
            held.append(int(spectra[-1].sum()))
        assert min(held) > 0  # both owners hold a part
        assert np.array_equal(spectra[0] + spectra[1], np.bincount(dump[3], minlength=256).astype(np.uint64))
        left = keep(dump, 2, 255)
        got = [[], [], [], []]
        for r in range(2):
            part = owners[r].enumerate(min_count=2, max_count=255)
            removed += owners[r].prune(2, 255)
            digests.append(owners[r].checksum())
            after = owners[r].enumerate()
            assert all(np.array_equal(x, y) for x, y in zip(part, after))
            for acc, x in zip(got, after):
                acc.append(x)
        for ix in owners:
            ix.close()
        want = O.digest_entries(*left)
        assert removed == len(dump[0]) - len(left[0])
        assert tuple((x + y) & 0xffffffffffffffff for x, y in zip(*digests)) == want
        assert same_multiset(tuple(np.concatenate(x) for x in got), left)
        O.index_free(h)


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(B):
    out = np.zeros(256, np.uint64)
    with B.BriskHip(31, 11, 4, entry_ids=True) as ix:
        assert ix.L.brisk_hip_count_spectrum(ix.h, out) == EINVAL
        assert ix.L.brisk_hip_prune(ix.h, 1, 255, None) == EINVAL
        assert raw_range(ix, 16, 0, 255)[0] == EINVAL
        with pytest.raises(B.BriskHipError):
            ix.count_spectrum()
    with B.BriskHip(31, 11, 4) as ix:
        ix.insert_reads(["ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGGCTAGCTAGCTAGGCTAGCCATAGACC"] * 3)
        cs = ix.checksum()
        assert ix.L.brisk_hip_prune(ix.h, 7, 3, None) == EINVAL
        assert raw_range(ix, 16, 7, 3)[0] == EINVAL
        L = ix.L
        saved = L.brisk_hip_count_spectrum.argtypes
        L.brisk_hip_count_spectrum.argtypes = [C.c_void_p, C.c_void_p]
        try:
            assert L.brisk_hip_count_spectrum(ix.h, None) == EINVAL  # a NULL out
        finally:
            L.brisk_hip_count_spectrum.argtypes = saved
        assert ix.L.brisk_hip_prune(ix.h, 0, 255, None) == 0  # `removed` may be NULL
        assert ix.checksum() == cs  # nothing above changed the index
        assert ix.prune(200, 255) == cs[0] and ix.checksum() == (0, 0, 0)
