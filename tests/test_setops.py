"""GPU: merge, intersect, subtract and compare of two indexes against the CPU oracle, bit-exact.

Expected values never come from the library under test: they are the oracle's index_dump of reads A and of reads B, joined in
Python on (hi, lo, idx), with Oracle.digest_entries for checksums and Oracle.bucket_ids for bucket counts; for merge also one
oracle index that received A and then B.  Where a test compares the library with itself (the order of the survivors, nb_skmers,
the algebra of checksums) it says so.

Geometries: the six of tests/test_spectrum_prune.py, plus k47 m13 b8 with part_bits = 4: thousands of entries in each of 16
partitions on both sides, so a partition of `src` is several table chunks of k_join (JN_ENT = 256 entries) and a partition of
`dst` several register blocks."""
import ctypes as C
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle
from test_gpu_parity import SPECIAL
from test_spectrum_prune import GEOM_IDS, GEOMS, largest_partition, oracle_index, partition_of, same_multiset, want_stats

pytestmark = pytest.mark.gpu

EINVAL = 1
TABLE_CHUNK = 256  # JN_ENT of brisk_setops.hip
ALL_GEOMS = GEOMS + [((47, 13, 8), dict(part_bits=4))]
ALL_IDS = GEOM_IDS + ["k47m13b8-pb4"]
RULES = {"left": lambda a, b: a, "min": min, "max": max, "sum": lambda a, b: (a + b) & 0xff}
COMPARE_KEYS = ("both", "only_self", "only_other", "sum_min", "sum_self", "sum_other")


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


def two_samples(seed, glen=6000, n_a=500, n_b=320):
    """A and B drawn from overlapping halves of one genome: A from [0, 2/3), B from [1/3, 1), both strands.  Different coverage,
    some reads repeated (other reads and other factors in A than in B), the low-complexity set in both."""
    rng = random.Random(seed)
    genome = "".join(rng.choice("ACGT") for _ in range(glen))
    rc = str.maketrans("ACGT", "TGCA")

    def draw(lo, hi, n, L=150):
        out = []
        for _ in range(n):
            p = rng.randrange(lo, hi - L)
            s = genome[p:p + L]
            out.append(s[::-1].translate(rc) if rng.random() < 0.5 else s)
        return out
    a = draw(0, 2 * glen // 3, n_a)
    b = draw(glen // 3, glen, n_b)
    a = a + a[:n_a // 3] * 2 + a[:30] * 6 + SPECIAL
    b = b + b[:n_b // 4] * 3 + SPECIAL * 2
    return a, b


def as_dict(dump):
    return {(h, l, i): c for l, h, i, c in zip(*(x.tolist() for x in dump))}


def as_dump(d):
    keys = list(d)
    return (np.array([x[1] for x in keys], np.uint64), np.array([x[0] for x in keys], np.uint64), np.array([x[2] for x in keys], np.uint8),
            np.array([d[x] for x in keys], np.uint8))


def expected(op, da, db, rule="left"):
    if op == "merge":
        out = dict(da)
        for key, c in db.items():
            out[key] = (out.get(key, 0) + c) & 0xff
        return out
    if op == "subtract":
        return {key: c for key, c in da.items() if key not in db}
    return {key: RULES[rule](c, db[key]) for key, c in da.items() if key in db}


def expected_compare(da, db):
    shared = [key for key in da if key in db]
    return dict(both=len(shared), only_self=len(da) - len(shared), only_other=len(db) - len(shared), sum_min=sum(min(da[x], db[x]) for x in shared),
                sum_self=sum(da[x] for x in shared), sum_other=sum(db[x] for x in shared))


def inputs(O, kmb, opts, seed_shift=0):
    k, m, b = kmb
    big = opts.get("part_bits") == 4
    reads_a, reads_b = two_samples(k * 100 + m + seed_shift, **(dict(glen=90000, n_a=4000, n_b=2600) if big else {}))
    ha, hb = oracle_index(O, reads_a, k, m, b), oracle_index(O, reads_b, k, m, b)
    da, db = as_dict(O.index_dump(ha)), as_dict(O.index_dump(hb))
    # the case tells an operation from a no-op and the count rules from each other -- asserted before the GPU is touched
    shared = [x for x in da if x in db]
    union = len(da) + len(db) - len(shared)
    assert min(len(shared), len(da) - len(shared), len(db) - len(shared)) * 10 >= union, (len(shared), len(da), len(db))
    assert sum(da[x] != db[x] for x in shared) * 10 >= len(shared)
    O.index_free(hb)
    return reads_a, reads_b, ha, da, db


def do(ix, other, op, rule):
    return ix.merge(other) if op == "merge" else ix.subtract(other) if op == "subtract" else ix.intersect(other, count=rule)


OPS = [("merge", "left"), ("subtract", "left"), ("intersect", "left"), ("intersect", "min"), ("intersect", "max"), ("intersect", "sum")]


# ---- 1: every operation, every geometry ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts", ALL_GEOMS, ids=ALL_IDS)
def test_operations_leave_the_expected_index(B, O, kmb, opts):
    k, m, b = kmb
    reads_a, reads_b, ha, da, db = inputs(O, kmb, opts)
    for op, rule in OPS:
        want = as_dump(expected(op, da, db, rule))
        with B.BriskHip(k, m, b, **opts) as ix, B.BriskHip(k, m, b, **opts) as src:
            ix.insert_reads(reads_a)
            src.insert_reads(reads_b)
            lay = ix.layout
            if opts.get("part_bits") == 4:  # the multi-chunk path of k_join is walked: on both sides
                for d in (da, db):
                    sizes = np.unique(partition_of(O, ha, as_dump(d), lay), return_counts=True)[1]
                    assert len(sizes) == 16 and sizes.max() > TABLE_CHUNK, sizes  # the largest partition exceeds the table chunk
            before, src_before, src_cs = ix.enumerate(), src.enumerate(), src.checksum()
            skm = ix.stats()["nb_skmers"], src.stats()["nb_skmers"]
            n = do(ix, src, op, rule)
            assert n == (len(want[0]) - len(da) if op == "merge" else len(da) - len(want[0])), (op, rule)
            after = ix.enumerate()
            assert same_multiset(after, want), (op, rule)
            st = ix.stats()
            assert (st["nb_kmers"], st["nb_buckets"]) == want_stats(O, ha, want), (op, rule)
            if lay["ext_bits"] == lay["cls_bits"]:
                assert st["largest_bucket"] == largest_partition(O, ha, want, lay), (op, rule)
            assert ix.checksum() == O.digest_entries(*want), (op, rule)
            assert np.array_equal(ix.count_spectrum(), np.bincount(want[3], minlength=256).astype(np.uint64)), (op, rule)
            # src is bit for bit what it was: same checksum, same enumeration, order included
            assert src.checksum() == src_cs and all(np.array_equal(x, y) for x, y in zip(src.enumerate(), src_before)), (op, rule)
            # the library against itself: nb_skmers, and the order of the entries that were there before
            assert st["nb_skmers"] == (skm[0] + skm[1] if op == "merge" else skm[0])
            if op != "merge":
                in_b = np.array([(h, l, i) in db for l, h, i in zip(*(x.tolist() for x in before[:3]))])
                mask = in_b if op == "intersect" else ~in_b
                assert all(np.array_equal(x, y[mask]) for x, y in zip(after[:3], before[:3])), (op, rule)  # survivors keep their relative order
    O.index_free(ha)


@pytest.mark.parametrize("kmb,opts", [ALL_GEOMS[0], ALL_GEOMS[1], ALL_GEOMS[6]], ids=[ALL_IDS[0], ALL_IDS[1], ALL_IDS[6]])
def test_merge_equals_one_index_that_received_both(B, O, kmb, opts):
    k, m, b = kmb
    reads_a, reads_b, ha, da, db = inputs(O, kmb, opts, seed_shift=5)
    hab = oracle_index(O, reads_a + reads_b, k, m, b)
    dump = O.index_dump(hab)
    assert same_multiset(as_dump(expected("merge", da, db)), dump)  # the join used above is the oracle's own result
    with B.BriskHip(k, m, b, **opts) as ix, B.BriskHip(k, m, b, **opts) as src:
        ix.insert_reads(reads_a)
        src.insert_reads(reads_b)
        assert ix.merge(src) == len(dump[0]) - len(da)
        assert ix.checksum() == O.index_digest(hab) and same_multiset(ix.enumerate(), dump)
        st = ix.stats()
        assert (st["nb_kmers"], st["nb_buckets"]) == O.index_stats(hab)
    O.index_free(ha)
    O.index_free(hab)


# ---- 2: compare ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts", ALL_GEOMS, ids=ALL_IDS)
def test_compare(B, O, kmb, opts):
    k, m, b = kmb
    reads_a, reads_b, ha, da, db = inputs(O, kmb, opts, seed_shift=1)
    with B.BriskHip(k, m, b, **opts) as a, B.BriskHip(k, m, b, **opts) as bb, B.BriskHip(k, m, b, **opts) as a2:
        a.insert_reads(reads_a)
        bb.insert_reads(reads_b)
        a2.insert_reads(reads_a[::-1])  # the same reads: the same entries in another storage order
        cs = a.checksum(), bb.checksum()
        got = a.compare(bb)
        assert tuple(got) == COMPARE_KEYS and got == expected_compare(da, db)
        swapped = bb.compare(a)
        assert swapped == expected_compare(db, da)
        same = a.compare(a2)
        total = sum(da.values())
        assert same == dict(both=len(da), only_self=0, only_other=0, sum_min=total, sum_self=total, sum_other=total)
        assert (a.checksum(), bb.checksum()) == cs and a2.checksum() == cs[0]  # neither checksum moves
    O.index_free(ha)


# ---- 3: counts that wrap ---------------------------------------------------------------------------------------------------------
def test_counts_wrap_and_a_count_of_zero_is_present(B, O):
    s = "ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGGCTAGCTAGCTAGGCTAGCCATAGACCAGATTTACAGGATACCCAGGGTAAACCA"
    z = "TTGACCGTAGGCTAACGGATTCAGGCATCGATACGGATCCATGGACTAGCATCGGATATCGCGATTAGCAGGACTTTACGCAGTAGCAAT"
    rng = random.Random(12)
    filler = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(60)]
    for k, m, b in ((63, 21, 14), (31, 15, 14)):
        reads_a = [s] * 200 + filler[:40]
        reads_b = [s] * 100 + [z] * 256 + filler[20:]
        ha, hb = oracle_index(O, reads_a, k, m, b), oracle_index(O, reads_b, k, m, b)
        da, db = as_dict(O.index_dump(ha)), as_dict(O.index_dump(hb))
        s_keys = [x for x in da if da[x] == 200]
        z_keys = [x for x in db if db[x] == 0]
        assert s_keys and z_keys and all(db[x] == 100 for x in s_keys) and not any(x in da for x in z_keys)

        def pair():
            ix, src = B.BriskHip(k, m, b), B.BriskHip(k, m, b)
            for i in range(0, len(reads_a), 50):
                ix.insert_reads(reads_a[i:i + 50])
            for i in range(0, len(reads_b), 50):
                src.insert_reads(reads_b[i:i + 50])
            return ix, src
        ix, src = pair()
        want = expected("merge", da, db)
        assert all(want[x] == 44 for x in s_keys) and all(want[x] == 0 for x in z_keys)  # 200 + 100 = 44 mod 256; 0 stays 0, and present
        assert ix.merge(src) == len(want) - len(da)
        assert same_multiset(ix.enumerate(), as_dump(want)) and ix.checksum() == O.digest_entries(*as_dump(want))
        lo, hi, idx = (np.array(v, dt) for v, dt in zip(zip(*[(x[1], x[0], x[2]) for x in z_keys]), (np.uint64, np.uint64, np.uint8)))
        data, found = ix.lookup(lo, hi, idx)
        assert found.all() and not data.any()
        # the merged index now holds the count-0 entries: subtract and intersect against src find them
        with B.BriskHip(k, m, b) as third:
            third.insert_reads(reads_a)
            third.merge(src)
            assert third.intersect(src, count="left") == len(want) - len(db)
            got = as_dict(third.enumerate())
            assert set(got) == set(db) and all(got[x] == 0 for x in z_keys)
        assert ix.subtract(src) == len(db)
        left = expected("subtract", da, db)
        assert same_multiset(ix.enumerate(), as_dump(left)) if left else len(ix.enumerate()[0]) == 0
        ix.close()
        src.close()
        O.index_free(ha)
        O.index_free(hb)


# ---- 4: the index afterwards -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts", ALL_GEOMS[:4], ids=ALL_IDS[:4])
def test_gets_and_inserts_after_an_operation(B, O, kmb, opts):
    """After each operation reads C go into dst; get_kmers and get_reads over reads of A, B and C then answer as the index of the
    expected entries plus C.  Expected per slot: the oracle's per-slot answers against its indexes of A, of B and of C (the same
    slot is the same identity in all three), combined by the operation's rule; slots inside spans that read the same on both
    strands are left out, and per-read sums are compared for reads whose oracle sum is the plain sum of their slots."""
    from test_kmer_query import expected_all
    k, m, b = kmb
    reads_a, reads_b, ha, da, db = inputs(O, kmb, opts, seed_shift=2)
    rng = random.Random(k)
    reads_c = reads_a[40:160] + reads_b[10:90] + ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(60)]
    hb, hc = oracle_index(O, reads_b, k, m, b), oracle_index(O, reads_c, k, m, b)
    dc = as_dict(O.index_dump(hc))
    queries = [q.upper() for q in reads_a[:120] + reads_b[:120] + reads_c[-100:]]
    hq = oracle_index(O, queries, k, m, b)
    qf, qo = oracle.pack_reads(queries)
    slots = {}
    ambiguous = None
    for name, h in (("a", ha), ("b", hb), ("c", hc), ("q", hq)):
        want, alts, base = expected_all(O, h, queries, k, m)
        slots[name] = ((want & 0x100) != 0, (want & 0xff).astype(np.int64))
        if ambiguous is None:
            ambiguous = np.zeros(len(want), bool)
        for s0, e0, _ in alts:
            ambiguous[s0:e0] = True
    seg = lambda v: np.array([int(v[int(base[r]):int(base[r + 1])].astype(np.int64).sum()) for r in range(len(queries))], np.uint64)
    plain = (seg(slots["q"][1] * slots["q"][0]) == O.index_query_reads(hq, qf, qo)) & (seg(ambiguous) == 0)
    assert plain.mean() > 0.8 and ambiguous.mean() < 0.2
    (fa, ca), (fb, cb), (fc, cc) = slots["a"], slots["b"], slots["c"]
    ca, cb, cc = ca * fa, cb * fb, cc * fc
    for op, rule in OPS:
        if op == "merge":
            f1, c1 = fa | fb, (ca + cb) & 0xff
        elif op == "subtract":
            f1, c1 = fa & ~fb, ca
        else:
            f1 = fa & fb
            c1 = {"left": ca, "min": np.minimum(ca, cb), "max": np.maximum(ca, cb), "sum": (ca + cb) & 0xff}[rule]
        c1 = np.where(f1, c1, 0)
        want_f, want_c = f1 | fc, (c1 + cc) & 0xff
        final = expected("merge", expected(op, da, db, rule), dc)
        with B.BriskHip(k, m, b, **opts) as ix, B.BriskHip(k, m, b, **opts) as src:
            ix.insert_reads(reads_a)
            src.insert_reads(reads_b)
            do(ix, src, op, rule)
            ix.insert_reads(reads_c)
            assert ix.checksum() == O.digest_entries(*as_dump(final)) and same_multiset(ix.enumerate(), as_dump(final)), (op, rule)
            st = ix.stats()
            assert (st["nb_kmers"], st["nb_buckets"]) == want_stats(O, ha, as_dump(final)), (op, rule)
            cnt, found, gbase = ix.get_kmers(queries)
            assert np.array_equal(gbase, base)
            ok = ~ambiguous
            assert np.array_equal(found[ok], want_f[ok]) and np.array_equal(cnt[ok].astype(np.int64), np.where(want_f, want_c, 0)[ok]), (op, rule)
            sums = ix.get_reads(queries)
            assert np.array_equal(sums[plain], seg(np.where(want_f, want_c, 0))[plain]), (op, rule)
            if op == "subtract":  # a k-mer removed by subtract and inserted again starts at 1: C's own count
                again = [x for x in dc if x in da and x in db]
                assert len(again) > 100 and all(final[x] == dc[x] for x in again)
                lo, hi, idx = (np.array(v, dt) for v, dt in zip(zip(*[(x[1], x[0], x[2]) for x in again]), (np.uint64, np.uint64, np.uint8)))
                data, fnd = ix.lookup(lo, hi, idx)
                assert fnd.all() and data.tolist() == [dc[x] for x in again]
    for h in (ha, hb, hc, hq):
        O.index_free(h)


# ---- 5: pending deferred inserts ---------------------------------------------------------------------------------------------------
def test_pending_inserts_of_both_sides_are_seen(B, O):
    k, m, b = 63, 21, 14
    reads_a, reads_b, ha, da, db = inputs(O, (k, m, b), {}, seed_shift=3)
    for op, rule in OPS + [("compare", "left")]:
        with B.BriskHip(k, m, b) as ix, B.BriskHip(k, m, b) as src:  # default options: these small batches are deferred
            for i in range(0, len(reads_a), 100):
                ix.insert_reads(reads_a[i:i + 100])
            for i in range(0, len(reads_b), 100):
                src.insert_reads(reads_b[i:i + 100])
            if op == "compare":  # no call in between on either side
                assert ix.compare(src) == expected_compare(da, db)
            else:
                do(ix, src, op, rule)
                assert ix.checksum() == O.digest_entries(*as_dump(expected(op, da, db, rule))), (op, rule)
            assert src.checksum() == O.digest_entries(*as_dump(db))
    O.index_free(ha)


# ---- 6: refusals (host-side checks that return before any launch) ----------------------------------------------------------------------
def test_refusals(B):
    reads = ["ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGGCTAGCTAGCTAGGCTAGCCATAGACCAGATTTACAGGATACCCAGGGTAAACCA"] * 3
    with B.BriskHip(31, 15, 8, part_bits=12) as ix:
        ix.insert_reads(reads)
        cs = ix.checksum()
        L, n, out = ix.L, C.c_uint64(), np.zeros(6, np.uint64)

        def all_refused(other, word):
            for rc in (L.brisk_hip_merge(ix.h, other.h, C.byref(n)), L.brisk_hip_intersect(ix.h, other.h, 0, C.byref(n)), L.brisk_hip_subtract(ix.h, other.h, C.byref(n)),
                       L.brisk_hip_compare(ix.h, other.h, out)):
                assert rc == EINVAL
                assert word in L.brisk_hip_last_error(ix.h).decode(), (word, L.brisk_hip_last_error(ix.h))
            assert ix.checksum() == cs
        for other_args, word in ((dict(k=31, m=13, b=8, part_bits=12), " m"), (dict(k=31, m=15, b=8, part_bits=13), "part_bits"), (dict(k=31, m=15, b=8, part_bits=12, entry_ids=True), "entry-id"),
                                 (dict(k=31, m=15, b=8, part_bits=12, n_owners=2), "sharded")):
            with B.BriskHip(**other_args) as other:
                if not other_args.get("entry_ids") and other_args.get("n_owners", 1) == 1:
                    other.insert_reads(reads)
                ocs = other.checksum() if not other_args.get("entry_ids") else None
                all_refused(other, word)
                with pytest.raises(B.BriskHipError):
                    ix.merge(other)
                if ocs is not None:
                    assert other.checksum() == ocs
        all_refused(ix, "different handles")  # dst == src
        with B.BriskHip(31, 15, 8, part_bits=12) as other:
            other.insert_reads(reads)
            assert L.brisk_hip_intersect(ix.h, other.h, 4, C.byref(n)) == EINVAL and "count_rule" in L.brisk_hip_last_error(ix.h).decode()
            assert ix.checksum() == cs and other.checksum() == cs
            with pytest.raises(ValueError):
                ix.intersect(other, count="both")
            # the counter pointers may be NULL
            assert L.brisk_hip_subtract(ix.h, other.h, None) == 0 and ix.checksum() == (0, 0, 0)
            assert L.brisk_hip_merge(ix.h, other.h, None) == 0 and ix.checksum() == cs
            assert L.brisk_hip_intersect(ix.h, other.h, 1, None) == 0 and ix.checksum() == cs


# ---- 7: algebra on the device (the library against itself; cheap, catches asymmetries) ------------------------------------------------
@pytest.mark.parametrize("kmb,opts", [ALL_GEOMS[0], ALL_GEOMS[2], ALL_GEOMS[6]], ids=[ALL_IDS[0], ALL_IDS[2], ALL_IDS[6]])
def test_algebra(B, kmb, opts):
    k, m, b = kmb
    reads_a, reads_b = two_samples(99, **(dict(glen=90000, n_a=4000, n_b=2600) if opts.get("part_bits") == 4 else {}))

    def index(reads):
        ix = B.BriskHip(k, m, b, **opts)
        ix.insert_reads(reads)
        return ix
    a, b1, a2, b2, a3, a4 = index(reads_a), index(reads_b), index(reads_a), index(reads_b), index(reads_a), index(reads_a)
    cs_a = a.checksum()
    a.merge(b1)
    b2.merge(a2)
    assert a.checksum() == b2.checksum()  # merge(A, B) and merge(B, A)
    shared = a3.subtract(b1)  # A \ B ...
    assert a4.intersect(b1, count="left") == cs_a[0] - shared  # ... and A AND B with A's counts ...
    assert 0 < shared < cs_a[0]
    assert a3.merge(a4) == shared and a3.checksum() == cs_a  # ... restore A
    for ix in (a, b1, a2, b2, a3, a4):
        ix.close()


# ---- 8: kernel variants, working density, the app ------------------------------------------------------------------------------------
def _worker(name, extra_env, timeout):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), name)
    env = {k: v for k, v in os.environ.items() if not k.startswith("BRISK_") or k == "BRISK_HIP_LIB"}
    env.update(extra_env)
    t0 = time.time()
    p = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=timeout)
    print(f"{name} {extra_env}: {time.time() - t0:.0f} s")
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout[-6000:], p.stderr[-6000:])


@pytest.mark.parametrize("env", [{"BRISK_INSERT_GENERIC": "1"}, {"BRISK_BINS": "0"}], ids=["insert-generic", "bins-0"])
def test_merge_under_kernel_variants(env):
    """merge's records through the run-time insert body, and with the binned scan off: tests/setops_worker.py variants"""
    _worker("setops_worker.py", dict(env, SETOPS_WORKER_CASE="variants"), 600)


def test_working_density():
    """two sets of ~400 k error-bearing reads, k63 m21 b14, default partitions: tests/setops_worker.py density"""
    _worker("setops_worker.py", dict(SETOPS_WORKER_CASE="density"), 900)


def _histo(path):
    return [int(line.split("\t")[1]) for line in open(path)]


def test_app_subtract_and_merge(B, tmp_path):
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "brisk_amd", "apps", "brisk_count")
    apps = {"brisk_count": exe} if os.path.exists(exe) else B.build_apps()
    fa = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test.fa")
    env = {k: v for k, v in os.environ.items() if not k.startswith("BRISK_") or k == "BRISK_HIP_LIB"}
    runs = {}
    for name, extra in (("plain", []), ("subtract", ["--subtract", fa]), ("merge", ["--merge", fa]), ("intersect", ["--intersect", fa])):
        out = str(tmp_path / (name + ".histo"))
        p = subprocess.run([apps["brisk_count"], "--bulk", fa, "31", "15", "14"] + extra + ["--histo", out], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.stdout, p.stderr)
        runs[name] = _histo(out), p.stderr, p.stdout
    plain = runs["plain"][0]
    total = sum(plain)
    assert total > 0 and len(plain) == 256 and max(c for c in range(256) if plain[c]) < 128
    assert not any(runs["subtract"][0]) and f"{total} entries removed" in runs["subtract"][1] and "nb_kmers 0 " in runs["subtract"][2]
    assert runs["merge"][0] == [plain[c // 2] if c % 2 == 0 else 0 for c in range(256)] and ": 0 entries added" in runs["merge"][1]  # every count doubled
    assert runs["intersect"][0] == plain and ": 0 entries removed" in runs["intersect"][1]
