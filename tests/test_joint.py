"""GPU: the joint count spectrum and the joint count-window filter of two indexes against the CPU oracle, bit-exact.

Expected values never come from the library under test: they are the oracle's index_dump of reads A and of reads B, joined in
Python on (hi, lo, idx) -- brisk_amd.joint_spectrum_from_entries over the two dumps for the matrix, a dict comprehension for the
filter -- with Oracle.digest_entries for checksums and Oracle.bucket_ids for bucket counts.  Where a test compares the library
with itself (marginals against count_spectrum, the present block against compare, a window against intersect / subtract / prune,
the order of the survivors) it says so.

Geometries and inputs: those of tests/test_setops.py (k47 m13 b8 with part_bits = 4 has partitions of several table chunks and
several register blocks on both sides), and every row of tests/geometry_edges.py with a smaller sample.  The filter windows run on
window_samples, inputs built so that every window removes and keeps at least a tenth of the entries."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from geometry_edges import TABLE, opts as row_opts, row_id
from test_setops import ALL_GEOMS, ALL_IDS, TABLE_CHUNK, as_dict, as_dump, inputs, two_samples
from test_spectrum_prune import largest_partition, oracle_index, partition_of, same_multiset, want_stats

pytestmark = pytest.mark.gpu

EINVAL = 1
A = 256       # BRISK_HIP_JOINT_ABSENT
TILE_T = 31   # JS_T of brisk_setops.hip: states below it (and absent) are counted in the wave's LDS tile, the others in global memory
# (min_self, max_self, min_other, max_other, keep_absent)
WINDOWS = [(0, 255, 0, 255, False), (0, 255, 1, 0, True), (2, 255, 0, 255, True), (2, 20, 0, 1, True), (1, 255, 3, 255, False), (5, 5, 0, 255, True)]
NO_OP = (0, 255, 0, 255, True)


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


# (times in A, times in B) of the segment classes of window_samples: every window of WINDOWS keeps some classes whole and removes others
CLASSES = [(1, 0), (1, 1), (5, 0), (5, 3), (2, 1), (3, 4), (1, 3), (33, 2), (5, 1), (40, 0), (0, 2), (0, 35)]


def window_samples(seed, per_class=12):
    """Reads for the windows.  test_setops.two_samples alone does not do: at k = 31 it leaves 2 % of A's entries with a count below 2
    and none at exactly 5, so (2,255,0,255,True) and (5,5,0,255,True) would be a no-op and a clear.  Here most entries come from
    disjoint 150-nt segments of a second random genome, segment j read CLASSES[j % 12] times into A and into B -- every k-mer of a
    segment then has exactly those counts -- on top of a small two_samples for mixed counts and the low-complexity set."""
    rng = random.Random(seed)
    a, b = two_samples(seed, glen=3000, n_a=200, n_b=130)
    for j in range(per_class * len(CLASSES)):
        seg = "".join(rng.choice("ACGT") for _ in range(150))
        na, nb = CLASSES[j % len(CLASSES)]
        a, b = a + [seg] * na, b + [seg] * nb
    rng.shuffle(a)
    rng.shuffle(b)
    return a, b


def window_inputs(O, kmb, seed_shift=0):
    k, m, b = kmb
    reads_a, reads_b = window_samples(k * 100 + m + seed_shift)
    ha, hb = oracle_index(O, reads_a, k, m, b), oracle_index(O, reads_b, k, m, b)
    da, db = as_dict(O.index_dump(ha)), as_dict(O.index_dump(hb))
    O.index_free(hb)
    return reads_a, reads_b, ha, da, db


def joint_of(B, da, db):
    """the yardstick: the definition in numpy, fed the oracle's entries"""
    return B.joint_spectrum_from_entries(as_dump(da), as_dump(db))


def passes(w, c, other):
    """the window on one entry: c its count, other its count in src or None"""
    lo, hi, olo, ohi, absent = w
    return lo <= c <= hi and (absent if other is None else olo <= other <= ohi)


def filtered(da, db, w):
    return {x: c for x, c in da.items() if passes(w, c, db.get(x))}


def in_order(before, keep_keys):
    mask = np.array([(h, l, i) in keep_keys for l, h, i in zip(*(x.tolist() for x in before[:3]))], bool)
    return tuple(x[mask] for x in before)


def same_arrays(xs, ys):
    return len(xs) == len(ys) and all(np.array_equal(x, y) for x, y in zip(xs, ys))


def check_joint(B, ix, src, da, db):
    """ix.joint_spectrum(src) against the Python join; then the library against itself: marginals, compare, nothing moved"""
    want = joint_of(B, da, db)
    state = ix.checksum(), src.checksum(), ix.enumerate(), src.enumerate()
    got = ix.joint_spectrum(src)
    assert got.shape == (257, 257) and got.dtype == np.uint64
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(sa), int(sb), int(got[sa, sb]), int(want[sa, sb])) for sa, sb in bad[:8]]
    assert got[A, A] == 0
    # the library against itself
    assert np.array_equal(got[:A].sum(axis=1), ix.count_spectrum()) and np.array_equal(got[:, :A].sum(axis=0), src.count_spectrum())
    cmp_, block, n = ix.compare(src), got[:A, :A].astype(object), np.arange(256, dtype=object)
    assert cmp_ == dict(both=int(block.sum()), only_self=int(got[:A, A].sum()), only_other=int(got[A, :A].sum()), sum_min=int((block * np.minimum.outer(n, n)).sum()),
                        sum_self=int((block.sum(axis=1) * n).sum()), sum_other=int((block.sum(axis=0) * n).sum()))
    assert (ix.checksum(), src.checksum()) == state[:2] and same_arrays(ix.enumerate(), state[2]) and same_arrays(src.enumerate(), state[3])
    return got


def check_filtered_index(O, ix, ha, want, removed, n_before, what):
    dump = as_dump(want)
    assert removed == n_before - len(want), what
    after = ix.enumerate()
    assert same_multiset(after, dump) if want else len(after[0]) == 0, what
    st, lay = ix.stats(), ix.layout
    assert (st["nb_kmers"], st["nb_buckets"]) == (want_stats(O, ha, dump) if want else (0, 0)), what
    if lay["ext_bits"] == lay["cls_bits"]:
        assert st["largest_bucket"] == largest_partition(O, ha, dump, lay), what
    assert ix.checksum() == O.digest_entries(*dump), what
    assert np.array_equal(ix.count_spectrum(), np.bincount(dump[3], minlength=256).astype(np.uint64)), what
    return after, st


# ---- 1: the joint spectrum, every geometry --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts", ALL_GEOMS, ids=ALL_IDS)
def test_joint_spectrum_equals_the_python_join(B, O, kmb, opts):
    k, m, b = kmb
    reads_a, reads_b, ha, da, db = inputs(O, kmb, opts)
    want = joint_of(B, da, db)
    # the case reaches the tile and the global bins, matched and unmatched -- asserted before the GPU is touched
    shared = [(c, db[x]) for x, c in da.items() if x in db]
    only_a = [c for x, c in da.items() if x not in db]
    assert np.count_nonzero(want) >= 300
    assert any(ca < TILE_T and cb < TILE_T for ca, cb in shared) and any(ca >= TILE_T or cb >= TILE_T for ca, cb in shared)
    assert any(c < TILE_T for c in only_a) and any(c >= TILE_T for c in only_a)
    with B.BriskHip(k, m, b, **opts) as ix, B.BriskHip(k, m, b, **opts) as src:
        ix.insert_reads(reads_a)
        src.insert_reads(reads_b)
        if opts.get("part_bits") == 4:  # the multi-chunk path is walked: on both sides
            for d in (da, db):
                sizes = np.unique(partition_of(O, ha, as_dump(d), ix.layout), return_counts=True)[1]
                assert len(sizes) == 16 and sizes.max() > TABLE_CHUNK, sizes  # the largest partition exceeds the table chunk
        got = check_joint(B, ix, src, da, db)
        assert np.array_equal(src.joint_spectrum(ix), got.T)  # (the library against itself: the other way round)
    O.index_free(ha)


# ---- 2: the key-layout boundary geometries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", TABLE, ids=[row_id(r) for r in TABLE])
def test_boundary_geometries(B, O, r):
    k, m, b = r.k, r.m, r.b
    reads_a, reads_b = two_samples(r.k * 10000 + r.m * 100 + r.b, glen=3000, n_a=200, n_b=130)
    ha, hb = oracle_index(O, reads_a, k, m, b), oracle_index(O, reads_b, k, m, b)
    da, db = as_dict(O.index_dump(ha)), as_dict(O.index_dump(hb))
    w = (2, 255, 0, 1, True)
    want = filtered(da, db, w)
    assert 0 < len(want) < len(da)
    with B.BriskHip(k, m, b, **row_opts(r)) as ix, B.BriskHip(k, m, b, **row_opts(r)) as src:
        ix.insert_reads(reads_a)
        src.insert_reads(reads_b)
        check_joint(B, ix, src, da, db)
        before, src_cs = ix.enumerate(), src.checksum()
        removed = ix.filter_joint(src, *w)
        assert removed == len(da) - len(want)
        assert ix.checksum() == O.digest_entries(*as_dump(want)) and same_arrays(ix.enumerate(), in_order(before, want))
        assert src.checksum() == src_cs
    O.index_free(ha)
    O.index_free(hb)


# ---- 3: states 0, 255 and absent ------------------------------------------------------------------------------------------------------
def test_states_0_255_and_absent(B, O):
    rng = random.Random(2024)
    X, Y, Z = ("".join(rng.choice("ACGT") for _ in range(150)) for _ in range(3))  # not drawn from the genome
    base_a, base_b = two_samples(7, glen=3000, n_a=200, n_b=130)
    reads_a = base_a + [X] * 256 + [Y] * 256 + [Z] * 300
    reads_b = base_b + [X] * 255 + [Y] * 256
    for k, m, b in ((63, 21, 14), (31, 15, 14)):
        dump_of = lambda reads: as_dict(O.index_dump(oracle_index(O, reads, k, m, b)))
        da, db = dump_of(reads_a), dump_of(reads_b)
        ba, bb, kx, ky, kz = (dump_of(x) for x in (base_a, base_b, [X], [Y], [Z]))
        assert all(c == 1 for d in (kx, ky, kz) for c in d.values()) and not (set(kx) | set(ky) | set(kz)) & (set(ba) | set(bb)) and not set(kx) & set(ky)
        assert max(ba.values()) < 255 and max(bb.values()) < 255
        # what every identity was seen, exactly; the oracle's wrapping dumps are these mod 256
        seen_a = {x: ba.get(x, 0) + 256 * (x in kx) + 256 * (x in ky) + 300 * (x in kz) for x in set(ba) | set(kx) | set(ky) | set(kz)}
        seen_b = {x: bb.get(x, 0) + 255 * (x in kx) + 256 * (x in ky) for x in set(bb) | set(kx) | set(ky)}
        assert {x: c & 0xff for x, c in seen_a.items()} == da and {x: c & 0xff for x, c in seen_b.items()} == db
        want = joint_of(B, da, db)
        assert want[0, 255] == len(kx) and want[0, 0] == len(ky) and want[44, A] >= len(kz) and not want[A, 255] and not want[A, 0]

        def pair(**kw):
            ix, src = B.BriskHip(k, m, b, **kw), B.BriskHip(k, m, b, **kw)
            for i in range(0, len(reads_a), 200):
                ix.insert_reads(reads_a[i:i + 200])
            for i in range(0, len(reads_b), 200):
                src.insert_reads(reads_b[i:i + 200])
            return ix, src
        ix, src = pair()
        got = check_joint(B, ix, src, da, db)
        assert got[0, 255] == len(kx) and got[0, 0] == len(ky) and got[44, A] == want[44, A] and not got[A, 255] and not got[A, 0]
        # the filters, wrapping: src's count exactly 255 is X alone; a stored count of 0 here is X and Y
        only_x = filtered(da, db, (0, 255, 255, 255, False))
        assert set(only_x) == set(kx)
        assert ix.filter_joint(src, min_other=255, max_other=255) == len(da) - len(kx)
        assert same_multiset(ix.enumerate(), as_dump(only_x)) and ix.checksum() == O.digest_entries(*as_dump(only_x))
        ix.close()
        src.close()
        ix, src = pair()
        x_and_y = filtered(da, db, (0, 0, 0, 255, True))
        assert set(x_and_y) == set(kx) | set(ky)
        assert ix.filter_joint(src, 0, 0, 0, 255, keep_absent=True) == len(da) - len(x_and_y)
        assert same_multiset(ix.enumerate(), as_dump(x_and_y)) and ix.checksum() == O.digest_entries(*as_dump(x_and_y))
        ix.close()
        src.close()
        # saturating on both handles: 255 is "255 or more", state 0 is empty on both axes
        sa, sb = {x: min(c, 255) for x, c in seen_a.items()}, {x: min(c, 255) for x, c in seen_b.items()}
        want = joint_of(B, sa, sb)
        assert want[255, 255] == len(kx) + len(ky) and want[255, A] == len(kz) and not want[0].any() and not want[:, 0].any()
        ix, src = pair(count_mode="saturate")
        got = check_joint(B, ix, src, sa, sb)
        assert got[255, 255] == len(kx) + len(ky) and got[255, A] == len(kz) and not got[0].any() and not got[:, 0].any()
        # a bound of 255 keeps everything seen at least 255 times
        assert ix.filter_joint(src, 255, 255, 255, 300, keep_absent=True) == len(sa) - len(kx) - len(ky) - len(kz)
        assert set(as_dict(ix.enumerate())) == set(kx) | set(ky) | set(kz)
        ix.close()
        src.close()


# ---- 4: empty indexes, pending deferred inserts ----------------------------------------------------------------------------------------
def test_empty_sides(B, O):
    k, m, b = 31, 15, 14
    reads = two_samples(11, glen=3000, n_a=200, n_b=130)[0]
    d = as_dict(O.index_dump(oracle_index(O, reads, k, m, b)))
    spectrum = np.bincount(as_dump(d)[3], minlength=256).astype(np.uint64)
    with B.BriskHip(k, m, b) as full, B.BriskHip(k, m, b) as e1, B.BriskHip(k, m, b) as e2:
        full.insert_reads(reads)
        J = full.joint_spectrum(e1)  # b empty: every entry in the column `absent`
        assert np.array_equal(J[:A, A], spectrum) and int(J.sum()) == len(d) and np.array_equal(J, joint_of(B, d, {}))
        J = e1.joint_spectrum(full)  # a empty: every entry in the row `absent`
        assert np.array_equal(J[A, :A], spectrum) and int(J.sum()) == len(d) and np.array_equal(J, joint_of(B, {}, d))
        assert not e1.joint_spectrum(e2).any()
        cs = full.checksum()
        assert e1.filter_joint(full) == 0 and e1.checksum() == (0, 0, 0)
        assert full.filter_joint(e1, keep_absent=True) == 0 and full.checksum() == cs  # nothing is in src: the self window alone, and it is full
        want = {x: c for x, c in d.items() if c >= 2}
        assert full.filter_joint(e1, min_self=2, keep_absent=True) == len(d) - len(want) and full.checksum() == O.digest_entries(*as_dump(want))
        assert full.filter_joint(e1) == len(want) and full.checksum() == (0, 0, 0) and full.stats()["nb_buckets"] == 0  # and without keep_absent it is emptied


def test_pending_inserts_of_both_sides_are_seen(B, O):
    k, m, b = 63, 21, 14
    reads_a, reads_b, ha, da, db = inputs(O, (k, m, b), {}, seed_shift=3)
    w = (2, 20, 0, 1, True)
    for call in ("joint_spectrum", "filter_joint"):
        with B.BriskHip(k, m, b) as ix, B.BriskHip(k, m, b) as src:  # default options: these small batches are deferred
            for i in range(0, len(reads_a), 100):
                ix.insert_reads(reads_a[i:i + 100])
            for i in range(0, len(reads_b), 100):
                src.insert_reads(reads_b[i:i + 100])
            if call == "joint_spectrum":  # no call in between on either side
                assert np.array_equal(ix.joint_spectrum(src), joint_of(B, da, db))
            else:
                want = filtered(da, db, w)
                assert ix.filter_joint(src, *w) == len(da) - len(want) and ix.checksum() == O.digest_entries(*as_dump(want))
            assert src.checksum() == O.digest_entries(*as_dump(db))
    O.index_free(ha)


# ---- 5: filter_joint leaves the expected index ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts", ALL_GEOMS, ids=ALL_IDS)
def test_filter_joint_leaves_the_expected_index(B, O, kmb, opts):
    k, m, b = kmb
    reads_a, reads_b, ha, da, db = window_inputs(O, kmb)
    for w in WINDOWS:  # no case is a no-op or a clear -- asserted before the GPU is touched
        n = len(filtered(da, db, w))
        assert n * 10 >= len(da) and (len(da) - n) * 10 >= len(da), (w, n, len(da))

    def pair():
        ix, src = B.BriskHip(k, m, b, **opts), B.BriskHip(k, m, b, **opts)
        ix.insert_reads(reads_a)
        src.insert_reads(reads_b)
        return ix, src
    for wi, w in enumerate(WINDOWS):
        want = filtered(da, db, w)
        ix, src = pair()
        if opts.get("part_bits") == 4 and wi == 0:  # partitions of several table chunks and register blocks, on both sides
            for d in (da, db):
                sizes = np.unique(partition_of(O, ha, as_dump(d), ix.layout), return_counts=True)[1]
                assert len(sizes) == 16 and sizes.min() > TABLE_CHUNK, sizes
        before, src_before, src_cs, skm = ix.enumerate(), src.enumerate(), src.checksum(), ix.stats()["nb_skmers"]
        removed = ix.filter_joint(src, *w)
        after, st = check_filtered_index(O, ix, ha, want, removed, len(da), w)
        # src is bit for bit what it was: same checksum, same enumeration, order included
        assert src.checksum() == src_cs and same_arrays(src.enumerate(), src_before), w
        # the library against itself: nb_skmers, and the survivors in the order they had -- counts included
        assert st["nb_skmers"] == skm and same_arrays(after, in_order(before, want)), w
        if wi < 3:  # the library against itself: the window that is intersect(left), subtract, prune(2, 255)
            ix2, src2 = pair()
            n2 = ix2.intersect(src2, count="left") if wi == 0 else ix2.subtract(src2) if wi == 1 else ix2.prune(2, 255)
            # (two handles that received the same reads need not store them in the same order: the multiset, not the order)
            assert n2 == removed and ix2.checksum() == ix.checksum() and same_multiset(ix2.enumerate(), after), w
            ix2.close()
            src2.close()
        ix.close()
        src.close()
    if kmb == ALL_GEOMS[0][0] and not opts:  # the deliberate no-op, once: nothing removed, nothing moved
        ix, src = pair()
        before, cs = ix.enumerate(), ix.checksum()
        assert ix.filter_joint(src, *NO_OP) == 0 and ix.checksum() == cs and same_arrays(ix.enumerate(), before)
        ix.close()
        src.close()
    O.index_free(ha)


# ---- 6: life after a filter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmb,opts", ALL_GEOMS[:4], ids=ALL_IDS[:4])
def test_gets_and_inserts_after_a_filter(B, O, kmb, opts):
    """get_kmers over reads of A after the filter: per slot, the oracle's answers against its indexes of A and of B (the same slot is
    the same identity in both) put through the window; slots inside spans that read the same on both strands are left out.  Then B's
    reads go in: the index is the oracle's `survivors, then B`."""
    from test_kmer_query import expected_all
    k, m, b = kmb
    reads_a, reads_b, ha, da, db = window_inputs(O, kmb, seed_shift=2)
    hb = oracle_index(O, reads_b, k, m, b)
    w = (2, 20, 0, 1, True)
    lo, hi, olo, ohi, _ = w
    queries = [q.upper() for q in reads_a[:150]]
    (sa, alts_a, base), (sb, alts_b, _) = expected_all(O, ha, queries, k, m), expected_all(O, hb, queries, k, m)
    ambiguous = np.zeros(len(sa), bool)
    for s0, e0, _ in alts_a + alts_b:
        ambiguous[s0:e0] = True
    fa, ca, fb, cb = (sa & 0x100) != 0, sa & 0xff, (sb & 0x100) != 0, sb & 0xff
    keep = fa & (ca >= lo) & (ca <= hi) & np.where(fb, (cb >= olo) & (cb <= ohi), True)
    ok = ~ambiguous
    assert ambiguous.mean() < 0.2 and keep[ok].any() and (fa & ~keep)[ok].any() and (keep & fb)[ok].any()
    want = filtered(da, db, w)
    final = dict(want)
    for x, c in db.items():
        final[x] = (final.get(x, 0) + c) & 0xff
    back = [x for x in da if x in db and x not in want]  # removed, and B brings them back: they start at B's count
    assert len(back) > 100 and all(final[x] == db[x] for x in back)
    with B.BriskHip(k, m, b, **opts) as ix, B.BriskHip(k, m, b, **opts) as src:
        ix.insert_reads(reads_a)
        src.insert_reads(reads_b)
        assert ix.filter_joint(src, *w) == len(da) - len(want)
        cnt, found, gbase = ix.get_kmers(queries)
        assert np.array_equal(gbase, base)
        assert np.array_equal(found[ok], keep[ok]) and np.array_equal(cnt[ok].astype(np.int64), np.where(keep, ca, 0)[ok])
        ix.insert_reads(reads_b)
        dump = as_dump(final)
        assert ix.checksum() == O.digest_entries(*dump) and same_multiset(ix.enumerate(), dump)
        st = ix.stats()
        assert (st["nb_kmers"], st["nb_buckets"]) == want_stats(O, ha, dump)
        lo_, hi_, idx_ = (np.array(v, dt) for v, dt in zip(zip(*[(x[1], x[0], x[2]) for x in back]), (np.uint64, np.uint64, np.uint8)))
        data, fnd = ix.lookup(lo_, hi_, idx_)
        assert fnd.all() and data.tolist() == [db[x] for x in back]
    O.index_free(ha)
    O.index_free(hb)


# ---- 7: refusals (host-side checks that return before any launch) ----------------------------------------------------------------------
def test_refusals(B):
    reads = ["ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGGCTAGCTAGCTAGGCTAGCCATAGACCAGATTTACAGGATACCCAGGGTAAACCA"] * 3
    from brisk_amd.hipapi import _JointWindow
    with B.BriskHip(31, 15, 8, part_bits=12) as ix:
        ix.insert_reads(reads)
        cs = ix.checksum()
        L, n, out = ix.L, C.c_uint64(7), np.zeros(257 * 257, np.uint64)
        good = _JointWindow(0, 255, 0, 255, 0, 0)

        def both_refused(other, word, w=good):
            for rc in (L.brisk_hip_joint_spectrum(ix.h, other.h, out.ctypes.data), L.brisk_hip_filter_joint(ix.h, other.h, C.byref(w), C.byref(n))):
                assert rc == EINVAL
                assert word in L.brisk_hip_last_error(ix.h).decode(), (word, L.brisk_hip_last_error(ix.h))
            assert ix.checksum() == cs and n.value == 7 and not out.any()
        for other_args, word in ((dict(k=31, m=13, b=8, part_bits=12), " m"), (dict(k=29, m=15, b=8, part_bits=12), " k"), (dict(k=31, m=15, b=8, part_bits=13), "part_bits"),
                                 (dict(k=31, m=15, b=8, part_bits=12, count_mode="saturate"), "count_mode"), (dict(k=31, m=15, b=8, part_bits=12, entry_ids=True), "entry-id"),
                                 (dict(k=31, m=15, b=8, part_bits=12, n_owners=2), "sharded")):
            with B.BriskHip(**other_args) as other:
                plain = not other_args.get("entry_ids") and other_args.get("n_owners", 1) == 1
                if plain:
                    other.insert_reads(reads)
                ocs = other.checksum() if not other_args.get("entry_ids") else None
                both_refused(other, word)
                with pytest.raises(B.BriskHipError):
                    ix.joint_spectrum(other)
                with pytest.raises(B.BriskHipError):
                    ix.filter_joint(other)
                if ocs is not None:
                    assert other.checksum() == ocs
        both_refused(ix, "different handles")  # dst == src
        with B.BriskHip(31, 15, 8, part_bits=12) as other:
            other.insert_reads(reads)
            for w, word in ((_JointWindow(3, 2, 0, 255, 1, 0), "min_self > max_self"), (_JointWindow(0, 255, 0, 255, 1, 1), "reserved"), (_JointWindow(0, 255, 1, 0, 0, 0), "nothing can pass")):
                assert L.brisk_hip_filter_joint(ix.h, other.h, C.byref(w), C.byref(n)) == EINVAL and word in L.brisk_hip_last_error(ix.h).decode(), word
                assert n.value == 7 and ix.checksum() == cs and other.checksum() == cs
            assert L.brisk_hip_filter_joint(ix.h, other.h, None, C.byref(n)) == EINVAL and "window" in L.brisk_hip_last_error(ix.h).decode()
            assert L.brisk_hip_joint_spectrum(ix.h, other.h, None) == EINVAL and "out" in L.brisk_hip_last_error(ix.h).decode()
            assert n.value == 7 and ix.checksum() == cs and other.checksum() == cs
            # the counter pointer may be NULL
            assert L.brisk_hip_filter_joint(ix.h, other.h, C.byref(_JointWindow(0, 255, 1, 0, 1, 0)), None) == 0 and ix.checksum() == (0, 0, 0)


# ---- 8: the app ------------------------------------------------------------------------------------------------------------------------
def test_app_joint_and_filter_joint(B, tmp_path):
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "brisk_amd", "apps", "brisk_count")
    apps = {"brisk_count": exe} if os.path.exists(exe) else B.build_apps()
    fa = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test.fa")
    env = {k: v for k, v in os.environ.items() if not k.startswith("BRISK_") or k == "BRISK_HIP_LIB"}

    def run(*extra):
        return subprocess.run([apps["brisk_count"], "--bulk", fa, "31", "15", "14"] + list(extra), env=env, capture_output=True, text=True, timeout=300)
    histo, joint = str(tmp_path / "plain.histo"), str(tmp_path / "joint.tsv")
    p = run("--joint", fa, "--joint-histo", joint, "--histo", histo)
    assert p.returncode == 0, (p.stdout, p.stderr)
    plain = [int(line.split("\t")[1]) for line in open(histo)]
    rows = [tuple(int(x) for x in line.split("\t")) for line in open(joint)]
    assert sum(plain) > 0 and rows == [(c, c, n) for c, n in enumerate(plain) if n]  # the same file twice: diagonal lines only, the --histo of the same run
    filtered_histo = str(tmp_path / "filtered.histo")
    p = run("--filter-joint", fa, "--window", "0:255:1:0:absent", "--histo", filtered_histo)
    assert p.returncode == 0 and f"{sum(plain)} entries removed" in p.stderr, (p.stdout, p.stderr)
    assert not any(int(line.split("\t")[1]) for line in open(filtered_histo))
    for bad in ("0:255:1:0", "3:2:0:255", "0:256:0:255", "0:255:0", "0:255:0:255:present", "-1:255:0:255", "a:b:c:d"):  # a usage error before any device work
        p = run("--filter-joint", fa, "--window", bad)
        assert p.returncode == 2 and "--window" in p.stderr, (bad, p.stderr)
