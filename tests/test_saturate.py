"""Saturating counts on the device (brisk_hip_options.count_mode = BRISK_HIP_COUNTS_SATURATE): an entry's
stored count is min(255, the times its identity was inserted) whatever the batching, the deferral, the kernel, the record layout
or the fold; the default mode still wraps.  The yardstick (tests/saturate_worker.py) is the oracle's exact count of a read set
whose counts stay below 256, multiplied by the number of times the set was inserted."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import oracle
import saturate_worker as S

pytestmark = pytest.mark.gpu

CONFIGS = S.CONFIGS
EINVAL = 1


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    assert brisk_amd.library_path()
    return brisk_amd


@pytest.fixture(scope="module")
def reads():
    return S.base_reads()


def _filled(B, reads, k, m, b, t, **kw):
    ix = B.BriskHip(k, m, b, **kw)
    ix.insert_reads(reads * t)
    return ix


# ---- the yardstick against today's behaviour, then 1. parity
@pytest.mark.parametrize("k,m,b", CONFIGS)
def test_the_yardstick_predicts_the_wrapping_default(B, O, reads, k, m, b):
    base, nb = S.yardstick(O, "B", reads, k, m, b)
    want = S.expected(base, 3, S.wrap)
    assert max(3 * c for c in base.values()) >= 256, "t = 3 must wrap somewhere"
    with _filled(B, reads, k, m, b, 3) as ix:
        S.check_index(ix, want, nb, k, (k, m, b))
        assert ix.layout.get("count_mode", 0) == 0


@pytest.mark.parametrize("t", S.TS)
@pytest.mark.parametrize("k,m,b", CONFIGS)
def test_parity_with_the_yardstick_whatever_the_batching(B, O, reads, k, m, b, t):
    base, nb = S.yardstick(O, "B", reads, k, m, b)
    want = S.expected(base, t)
    n255 = sum(1 for c in base.values() if t * c >= 255)
    cuts = S.seven_cuts(reads * t, 7 * t + k)
    batchings = {"one call": ([reads * t], {}), "a call per copy": ([reads] * t, {}), "seven calls, deferred": (cuts, {}),
                 "seven calls, immediate": (cuts, {"immediate_inserts": True})}
    if t == 5:  # 16 partitions: each takes many chunks, and the running count crosses 255 between chunks and between calls
        batchings["part_bits 4, a call per copy"] = ([reads] * t, {"part_bits": 4})
        batchings["part_bits 4, seven calls"] = (cuts, {"part_bits": 4, "immediate_inserts": True})
    for name, (calls, kw) in batchings.items():
        with B.BriskHip(k, m, b, count_mode="saturate", **kw) as ix:
            assert ix.count_mode == "saturate" and ix.layout["count_mode"] == 1
            for part in calls:
                ix.insert_reads(part)
            S.check_index(ix, want, nb, k, (k, m, b, t, name))
            spec = ix.count_spectrum()
            assert spec[0] == 0 and spec[255] == n255, (name, spec[0], spec[255], n255)
    if t == 5:
        assert n255 > 0


# ---- 2. the record collapse and a header multiplicity above 255
@pytest.mark.parametrize("k,m,b", CONFIGS)
def test_one_read_300_times_and_300_more(B, O, reads, k, m, b):
    one, nb = S.yardstick(O, "one", reads[:1], k, m, b)
    want = {ident: 255 for ident in one}
    for kw in ({}, {"immediate_inserts": True}):  # (300 records a partition: the 512-instance kernel and its in-place collapse)
        with B.BriskHip(k, m, b, count_mode="saturate", **kw) as ix:
            for _ in range(2):
                ix.insert_reads(reads[:1] * 300)
                S.check_index(ix, want, nb, k, (k, m, b, kw))


# ---- 3. the kernels: every variant in a process of its own (the library reads the variables once)
@pytest.fixture(scope="module")
def parent_digest(B, O):
    return S.run_cases(B, O)


@pytest.mark.parametrize("extra", [{"BRISK_INSERT_GENERIC": "1"}, {"BRISK_HUGE_AT": "64"}, {"BRISK_INSERT_BIG_AT": "0", "BRISK_BINS": "0"}, {"BRISK_BINS": "0"},
                                   {"BRISK_BINS": "8"}], ids=["generic", "huge-at-64", "big-at-0", "bins-0", "bins-8"])
def test_every_insert_kernel_saturates_alike(parent_digest, extra):
    worker = os.path.join(ROOT, "tests", "saturate_worker.py")
    clean = {n: v for n, v in os.environ.items() if n not in ("BRISK_INSERT_GENERIC", "BRISK_HUGE_AT", "BRISK_INSERT_BIG_AT", "BRISK_BINS")}
    p = subprocess.run([sys.executable, worker], env=dict(clean, **extra), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (extra, p.stdout[-2000:], p.stderr[-4000:])
    assert p.stdout.strip().splitlines()[-1] == "digest " + parent_digest, extra


# ---- 4. where nothing reaches 256 the two modes are one
@pytest.mark.parametrize("k,m,b", CONFIGS)
def test_below_256_both_modes_agree(B, reads, k, m, b):
    with _filled(B, reads, k, m, b, 1) as w, _filled(B, reads, k, m, b, 1, count_mode="saturate") as s:
        assert w.count_mode == "wrap" and s.count_mode == "saturate"
        assert w.checksum() == s.checksum()
        assert w.count_spectrum().tolist() == s.count_spectrum().tolist()


# ---- 5. set operations, reallocate, compare
def _other_reads(reads):
    """B': the windows of the first half of the locus once more (shared with B), and a second locus (not in B)"""
    g2 = S.rand_seq(random.Random(808), 160)
    return reads[:150] + [g2[o:o + 100] for o in range(0, 61, 4)] * 2


def _counts_of(ix, k):
    out = {}
    for line in oracle.multiset_lines(*ix.enumerate(), k):
        w = line.split()
        out[(w[0], int(w[1]))] = int(w[2])
    return out


@pytest.mark.parametrize("k,m,b", CONFIGS)
def test_set_operations_between_saturating_indexes(B, O, reads, k, m, b):
    other = _other_reads(reads)
    ca, _ = S.yardstick(O, "B", reads, k, m, b)
    cb, _ = S.yardstick(O, "other", other, k, m, b)
    ta, tb = 2, 2
    a = {i: S.clamp(ta * c) for i, c in ca.items()}
    bb = {i: S.clamp(tb * c) for i, c in cb.items()}
    shared = set(a) & set(bb)
    assert shared and set(bb) - set(a) and set(a) - set(bb)
    assert any(a[i] + bb[i] > 255 and a[i] < 255 and bb[i] < 255 for i in shared), "a sum must cross 255 between two counts that have not"
    nb_union = S.nb_buckets(O, "union", reads + other, k, m, b)

    def pair():
        return _filled(B, reads, k, m, b, ta, count_mode="saturate"), _filled(B, other, k, m, b, tb, count_mode="saturate")

    # merge: min(255, a + b) on shared entries; src bit for bit unchanged
    dst, src = pair()
    with dst, src:
        assert _counts_of(dst, k) == a and _counts_of(src, k) == bb
        src_ck = src.checksum()
        added = dst.merge(src)
        want = {i: S.clamp(a.get(i, 0) + bb.get(i, 0)) for i in set(a) | set(bb)}
        assert added == len(set(bb) - set(a))
        S.check_index(dst, want, nb_union, k, "merge")
        assert src.checksum() == src_ck and _counts_of(src, k) == bb
        assert dst.count_spectrum()[0] == 0
    # intersect under every rule
    rules = {"sum": lambda x, y: S.clamp(x + y), "min": min, "max": max, "left": lambda x, y: x}
    for rule, f in rules.items():
        dst, src = pair()
        with dst, src:
            src_ck = src.checksum()
            removed = dst.intersect(src, count=rule)
            assert removed == len(set(a) - shared)
            assert _counts_of(dst, k) == {i: f(a[i], bb[i]) for i in shared}, rule
            assert src.checksum() == src_ck
    # subtract and compare
    dst, src = pair()
    with dst, src:
        cmp_ = dst.compare(src)
        assert cmp_ == {"both": len(shared), "only_self": len(set(a) - shared), "only_other": len(set(bb) - shared),
                        "sum_min": sum(min(a[i], bb[i]) for i in shared), "sum_self": sum(a[i] for i in shared), "sum_other": sum(bb[i] for i in shared)}
        assert dst.subtract(src) == len(shared)
        assert _counts_of(dst, k) == {i: c for i, c in a.items() if i not in shared}


@pytest.mark.parametrize("k,m,b", CONFIGS)
def test_a_wrapping_and_a_saturating_index_do_not_combine(B, reads, k, m, b):
    with _filled(B, reads, k, m, b, 1) as w, _filled(B, reads[:90], k, m, b, 1, count_mode="saturate") as s:
        cks = (w.checksum(), s.checksum())
        for x, y in ((w, s), (s, w)):
            calls = (lambda: x.merge(y), lambda: x.intersect(y), lambda: x.intersect(y, count="sum"), lambda: x.subtract(y), lambda: x.compare(y))
            for call in calls:
                with pytest.raises(B.BriskHipError) as e:
                    call()
                assert e.value.code == EINVAL and "count_mode" in str(e.value)
            with B.BriskHip(k, m + 2, b + 2, count_mode=y.count_mode) as fresh:
                with pytest.raises(B.BriskHipError) as e:
                    x.reallocate_into(fresh)
                assert e.value.code == EINVAL and "count_mode" in str(e.value)
                assert fresh.checksum()[0] == 0
        assert (w.checksum(), s.checksum()) == cks


@pytest.mark.parametrize("k,m,b", CONFIGS)
def test_reallocate_of_a_saturating_index(B, O, reads, k, m, b):
    """every entry goes to the identity the enumerator gives its k-mer at m + 2 (tests/test_reallocate.py); entries that merge add
    up and stop at 255"""
    base, _ = S.yardstick(O, "B", reads, k, m, b)
    t = 3  # (the largest count is 94 at k = 63 and 210 at k = 31: three copies take it past 255)
    old = S.expected(base, t)
    want, true = {}, {}
    for (km, _idx), c in base.items():
        _, _, lo, hi, idx, _ = O.enumerate(km, k, m + 2)
        assert len(lo) == 1
        ident = (oracle.kmer2str(int(lo[0]), int(hi[0]), k), int(idx[0]))
        true[ident] = true.get(ident, 0) + t * c
        want[ident] = S.clamp(want.get(ident, 0) + old[(km, _idx)])
    assert want == {i: S.clamp(v) for i, v in true.items()} and max(true.values()) > 255, "the input must cross 255"
    for pb in (0, 4):  # (few partitions: the 512-instance kernel collapses one-k-mer records that carry their counts)
        with _filled(B, reads, k, m, b, t, count_mode="saturate") as ix, B.BriskHip(k, m + 2, b + 2, count_mode="saturate", part_bits=pb) as fresh:
            ck = ix.checksum()
            ix.reallocate_into(fresh)
            got = _counts_of(fresh, k)
            assert got == want and max(got.values()) == 255 and min(got.values()) >= 1, pb
            assert fresh.count_spectrum()[0] == 0 and ix.checksum() == ck


# ---- 6. snapshots
@pytest.mark.parametrize("k,m,b", CONFIGS)
def test_snapshots_carry_the_mode(B, O, reads, tmp_path, k, m, b):
    base, nb = S.yardstick(O, "B", reads, k, m, b)
    t = 2
    sat, dflt = str(tmp_path / "sat.snap"), str(tmp_path / "wrap.snap")
    with _filled(B, reads, k, m, b, t, count_mode="saturate") as ix:
        ck = ix.checksum()
        ix.save(sat)
    raw = open(sat, "rb").read(256)
    assert raw[112] == 1 and raw[113:256] == bytes(143)
    assert B.snapshot_info(sat)["count_mode"] == 1
    with B.BriskHip.open(sat, room=True) as ld:
        assert ld.count_mode == "saturate" and ld.checksum() == ck
        ld.insert_reads(reads)
        S.check_index(ld, S.expected(base, t + 1), nb, k, "open + insert")
    with _filled(B, reads, k, m, b, t) as ix:
        ix.save(dflt)
    assert open(dflt, "rb").read(256)[112:256] == bytes(144)
    assert B.snapshot_info(dflt)["count_mode"] == 0
    with B.BriskHip.open(dflt) as ld:
        assert ld.count_mode == "wrap"
    # across the modes, both ways: EINVAL, the field named, the handle empty and usable
    for path, mode in ((sat, "wrap"), (dflt, "saturate")):
        with B.BriskHip(k, m, b, count_mode=mode) as ix:
            with pytest.raises(B.BriskHipError) as e:
                ix.load(path)
            assert e.value.code == EINVAL and "count_mode" in str(e.value)
            assert ix.checksum() == (0, 0, 0) and ix.stats()["nb_kmers"] == 0
            ix.insert_reads(reads)
            S.check_index(ix, S.expected(base, 1), nb, k, "after a refused load")


# ---- 7. the readers of the count
@pytest.mark.parametrize("k,m,b", CONFIGS)
def test_get_kmers_read_profile_and_prune(B, O, reads, k, m, b):
    base, nb = S.yardstick(O, "B", reads, k, m, b)
    def lost_at(t):
        return [i for i, c in base.items() if t * c >= 2 and (t * c) % 256 in (0, 1)]
    # t = 5 unless no identity's count comes round to 0 or 1 there (such an input shows nothing): then the next t that has one
    t = next(t for t in range(5, 40) if lost_at(t))
    lost = lost_at(t)
    want = S.expected(base, t)
    with _filled(B, reads, k, m, b, t, count_mode="saturate") as ix, _filled(B, reads, k, m, b, t) as wr:
        counts, found, slot_base = ix.get_kmers(reads)
        # a window's k-mers are the locus' k-mers: every slot is present, and its count is one of the index's; per read the
        # multiset of slot counts is what the yardstick gives the read's own identities
        assert found.all() and counts.min() >= 1
        wcounts, wfound, _ = wr.get_kmers(reads)
        assert wfound.all()
        for r in range(3):
            mine = sorted(counts[slot_base[r]:slot_base[r + 1]].tolist())
            one, _ = S.yardstick(O, ("read", r), reads[r:r + 1], k, m, b)
            assert mine == sorted(want[i] for i, c in one.items() for _ in range(c)), r
        # the wrapping index's slots are the same counts mod 256 wherever the true count is below 255
        low = counts < 255
        assert np.array_equal(wcounts[low], counts[low])
        for solid_min in (0, 2, 255):
            prof = ix.read_profile(reads, solid_min=solid_min)
            assert np.array_equal(prof, B.profile_from_slots(counts, found, slot_base, solid_min)), solid_min
        # prune(2, 255): the saturating index keeps every identity seen at least twice, the wrapping one loses those whose count
        # came round to 0 or 1 -- the reason the mode exists
        keep = {i: c for i, c in want.items() if t * base[i] >= 2}
        assert ix.prune(2, 255) == len(want) - len(keep)
        assert _counts_of(ix, k) == keep
        wkeep = {i: S.wrap(t * c) for i, c in base.items() if S.wrap(t * c) >= 2}
        assert wr.prune(2, 255) == len(base) - len(wkeep)
        assert _counts_of(wr, k) == wkeep
        assert set(keep) - set(wkeep) == set(lost) and lost


# ---- 8. the records path
@pytest.mark.parametrize("k,m,b", CONFIGS)
def test_records_path_and_two_owners(B, O, reads, k, m, b):
    import torch
    base, nb = S.yardstick(O, "B", reads, k, m, b)
    t = 3
    want = S.expected(base, t)
    flat, offs = oracle.pack_reads(reads * t)
    n = len(reads) * t
    with B.BriskHip(k, m, b, count_mode="saturate") as packed, B.BriskHip(k, m, b, count_mode="saturate", n_owners=1) as one:
        d_bases = torch.from_numpy(flat).cuda()
        d_packed = torch.zeros((len(flat) + 15) // 16 + 4, dtype=torch.int32, device="cuda")
        d_starts = torch.from_numpy(offs.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        packed.pack_ascii(d_bases.data_ptr(), len(flat), d_packed.data_ptr())
        packed.sync()
        packed.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
        S.check_index(packed, want, nb, k, "insert_packed")
        W = one.record_words
        bound = one.scan_bound(d_starts.data_ptr(), n)
        d_rec = torch.zeros(max(bound, 1) * W, dtype=torch.int64, device="cuda")
        d_out = torch.zeros_like(d_rec)
        torch.cuda.synchronize()
        n_rec = one.scan_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_rec.data_ptr(), bound)
        one.insert_records(d_rec.data_ptr(), n_rec)
        S.check_index(one, want, nb, k, "scan_packed -> insert_records")
        owners = [B.BriskHip(k, m, b, count_mode="saturate", owner_rank=r, n_owners=2) for r in range(2)]
        try:
            n_rec = owners[0].scan_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_rec.data_ptr(), bound)
            counts = owners[0].route_records(d_rec.data_ptr(), n_rec, d_out.data_ptr())
            o0 = int(counts[0])
            assert int(counts.sum()) == n_rec
            owners[0].insert_records(d_out.data_ptr(), o0)
            owners[1].insert_records(d_out[o0 * W:].data_ptr(), n_rec - o0)
            cks = [o.checksum() for o in owners]
            specs = [o.count_spectrum() for o in owners]
            M = (1 << 64) - 1
            assert tuple((x + y) & M for x, y in zip(*cks)) == packed.checksum()
            assert (specs[0] + specs[1]).tolist() == packed.count_spectrum().tolist()
            assert all(o.count_mode == "saturate" for o in owners)
        finally:
            for o in owners:
                o.close()


# ---- 9. refusals (return codes only)
def test_refusals(B):
    import ctypes as C
    from brisk_amd import hipapi
    L = hipapi.load()
    coef = hipapi.coef_table(21)
    for kw in ({"count_mode": 2}, {"count_mode": 7}, {"count_mode": 1, "entry_ids": 1}):
        opt = hipapi._Options(struct_size=C.sizeof(hipapi._Options), n_owners=1, **kw)
        h = C.c_void_p()
        rc = L.brisk_hip_create(C.byref(h), 63, 21, 14, 1, coef.ctypes.data_as(C.POINTER(C.c_double)), C.byref(opt))
        assert rc == EINVAL and not h.value, kw
    with pytest.raises(ValueError):
        B.BriskHip(63, 21, 14, count_mode="clamp")
    with pytest.raises(B.BriskHipError) as e:
        B.BriskHip(63, 21, 14, count_mode="saturate", entry_ids=True)
    assert e.value.code == EINVAL
    # a caller that passes the options as they were before the field existed gets the wrapping index
    opt = hipapi._Options(struct_size=hipapi._Options.count_mode.offset, n_owners=1, count_mode=1)
    h = C.c_void_p()
    assert L.brisk_hip_create(C.byref(h), 63, 21, 14, 1, coef.ctypes.data_as(C.POINTER(C.c_double)), C.byref(opt)) == 0
    lay = hipapi._Layout()
    assert L.brisk_hip_get_layout(h, C.byref(lay)) == 0 and lay.count_mode == 0
    assert L.brisk_hip_destroy(h) == 0
