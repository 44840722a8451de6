"""GPU: paired-end reads.  Every expectation is built from the numpy definitions (intervals_from_fragments, pair_intervals,
compose_intervals, split_pairs) and from extract_reference, never from the code under test: the four interval kernels row by row,
brisk_hip_extract_pairs_packed word for word against extract_reference over split_pairs' two tables, the composed calls
(trim_pairs_*, clean_pairs_*) against the host route, and brisk_count --paired against Python slicing of its inputs."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

from extract_reference import extract_reference, pack_reads
from extract_worker import E2E_GEOMETRIES, FILL, OutBuffers, device_reads, error_reads
from intake_reference import invalid_run
from test_extract import gather_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = 1, 5
ONES = np.uint64(2**64 - 1)
FILL_IV = 0x77777777


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    assert brisk_amd.library_path()
    return brisk_amd


def to_device(a):
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8)
    t = torch.from_numpy(raw if len(raw) else np.zeros(8, np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def iv_array(B, rows):
    return np.array(rows, np.uint32).reshape(-1, 2).copy().view(B.READ_INTERVAL_DTYPE).reshape(-1)


def filled_intervals(n):
    import torch
    t = torch.full((max(n, 1) * 2 + 2,), FILL_IV, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return t


def host_intervals(B, t, n):
    """(the first n rows, whether everything behind them still holds the fill)"""
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy().view(np.uint32)
    return a[:2 * n].copy().view(B.READ_INTERVAL_DTYPE), bool((a[2 * n:] == FILL_IV).all())


def four_states(B, intervals, at_least=20):
    c = B.split_pairs(intervals)[2]
    assert min(c["n_pairs_kept"], c["n_single_first"], c["n_single_second"], c["n_pairs_dropped"]) >= at_least, c
    return c


# ---- fragment_intervals -----------------------------------------------------------------------------------------------------------
def fragment_table(B, n_reads=600):
    rng = random.Random(600)
    rows = []
    for r in range(n_reads):
        if r in (0, n_reads - 1) or 100 <= r < 131 or 257 <= r < 300:
            n = 0
        elif r == 300:
            n = 70
        else:
            n = rng.choice((0, 1, 1, 2, 3, 5))
        at = rng.randint(0, 9)
        tie = rng.random() < 0.4
        length = rng.randint(5, 40)
        for _ in range(n):
            if not tie:
                length = rng.randint(5, 40)
            rows.append((r, at, length))
            at += length + rng.randint(1, 6)
    return np.array(rows, B.FRAGMENT_DTYPE)


def test_fragment_intervals(B):
    n_reads = 600
    frags = fragment_table(B, n_reads)
    want = B.intervals_from_fragments(frags, n_reads)
    per_read = np.bincount(frags["read"].astype(np.int64), minlength=n_reads)
    assert per_read[0] == 0 and per_read[-1] == 0 and per_read[300] == 70 and not per_read[100:131].any()
    ties = 0
    for r in np.nonzero(per_read >= 2)[0]:
        lens = frags["len"][frags["read"] == r]
        if (lens == lens.max()).sum() >= 2:
            ties += 1
            assert want[r]["start"] == frags["start"][frags["read"] == r][np.argmax(lens)]
    assert ties >= 20
    with B.BriskHip(31, 11, 11) as ix:
        d_frags = to_device(frags)
        d_iv = filled_intervals(n_reads)
        ix.fragment_intervals(d_frags.data_ptr(), len(frags), n_reads, d_iv.data_ptr())
        got, clean = host_intervals(B, d_iv, n_reads)
        assert np.array_equal(got, want), int(np.nonzero(got != want)[0][0])
        assert clean
        # no fragments at all: every row {0, 0}
        d_iv = filled_intervals(n_reads)
        ix.fragment_intervals(0, 0, n_reads, d_iv.data_ptr())
        got, clean = host_intervals(B, d_iv, n_reads)
        assert not got["start"].any() and not got["len"].any() and clean
        ix.fragment_intervals(0, 0, 0, 0)
        # a table with fewer reads than lanes in a wave
        few = frags[frags["read"] < 5]
        d_iv = filled_intervals(5)
        d_arg0 = to_device(few)   # (held until the call returns)
        ix.fragment_intervals(d_arg0.data_ptr(), len(few), 5, d_iv.data_ptr())
        assert np.array_equal(host_intervals(B, d_iv, 5)[0], B.intervals_from_fragments(few, 5))

        def refused(table, row):
            d_iv = filled_intervals(n_reads)
            with pytest.raises(B.BriskHipError) as e:
                d_arg0 = to_device(table)   # (held until the call returns)
                ix.fragment_intervals(d_arg0.data_ptr(), len(table), n_reads, d_iv.data_ptr())
            assert e.value.code == EINVAL and "row %d " % row in str(e.value), str(e.value)
            assert host_intervals(B, d_iv, 0)[1], "a refused call wrote to its output"
            with pytest.raises(ValueError):
                B.intervals_from_fragments(table, n_reads)

        bad = frags.copy()
        last_of_598 = int(np.nonzero(frags["read"] == frags["read"].max())[0][-1])
        bad[last_of_598]["read"] = n_reads          # read == n_reads, in order
        refused(bad, last_of_598)
        bad[17]["read"] = n_reads + 5               # two bad rows: the first is named
        refused(bad, 17)
        j = int(np.nonzero(per_read >= 2)[0][3])
        at = int(np.nonzero(frags["read"] == j)[0][0])
        bad = frags.copy()
        bad[[at, at + 1]] = bad[[at + 1, at]]       # two rows of one read swapped
        refused(bad, at + 1)
        at = int(np.nonzero(frags["read"] == 301)[0][0]) if per_read[301] else int(np.nonzero(frags["read"] > 301)[0][0])
        bad = frags.copy()
        bad[[at - 1, at]] = bad[[at, at - 1]]       # rows of two reads swapped
        refused(bad, at)
        assert ix.L.brisk_hip_fragment_intervals(ix.h, None, 3, n_reads, d_iv.data_ptr()) == EINVAL
        assert ix.L.brisk_hip_fragment_intervals(ix.h, d_frags.data_ptr(), len(frags), n_reads, None) == EINVAL


# ---- pair_intervals ---------------------------------------------------------------------------------------------------------------
def random_intervals(B, n, seed, p_keep=0.55):
    rng = np.random.default_rng(seed)
    v = np.zeros(n, B.READ_INTERVAL_DTYPE)
    v["start"] = rng.integers(0, 60, n)              # (a dropped row may carry a start)
    v["len"] = np.where(rng.random(n) < p_keep, rng.integers(1, 150, n), 0)
    return v


def test_pair_intervals(B):
    n = 600
    each, whole = random_intervals(B, n, 1), random_intervals(B, n, 2, 0.8)
    four_states(B, each)
    k = (each["len"] > 0).reshape(-1, 2).any(axis=1)
    w = (whole["len"] > 0).reshape(-1, 2)
    assert (k & ~w[:, 0]).sum() >= 20 and (k & ~w[:, 1]).sum() >= 20 and (k & w.all(axis=1)).sum() >= 20
    with B.BriskHip(31, 11, 11) as ix:
        d_each, d_whole = to_device(each), to_device(whole)
        for mode in ("each", "all", "any"):
            want = B.pair_intervals(each, whole, mode)
            d_out = filled_intervals(n)
            ix.pair_intervals(d_each.data_ptr(), d_whole.data_ptr() if mode == "any" else None, n, mode, d_out.data_ptr())
            got, clean = host_intervals(B, d_out, n)
            assert np.array_equal(got, want), (mode, int(np.nonzero(got != want)[0][0]))
            assert clean
            d_alias = to_device(each)                # d_out == d_each
            ix.pair_intervals(d_alias.data_ptr(), d_whole.data_ptr(), n, mode, d_alias.data_ptr())
            assert np.array_equal(d_alias.cpu().numpy().view(B.READ_INTERVAL_DTYPE), want), mode
        assert np.array_equal(host_intervals(B, d_each, n)[0], each)
        ix.pair_intervals(0, 0, 0, "all", 0)
        d_out = filled_intervals(n)
        for args, word in (((d_each.data_ptr(), d_whole.data_ptr(), n - 1, 0, d_out.data_ptr()), "odd"), ((d_each.data_ptr(), d_whole.data_ptr(), n, 3, d_out.data_ptr()), "pair_mode"),
                           ((d_each.data_ptr(), None, n, 2, d_out.data_ptr()), "d_whole")):
            assert ix.L.brisk_hip_pair_intervals(ix.h, *args) == EINVAL
            assert word in ix.L.brisk_hip_last_error(ix.h).decode()
        assert host_intervals(B, d_out, 0)[1]


# ---- compose_intervals ------------------------------------------------------------------------------------------------------------
def test_compose_intervals(B):
    rng = random.Random(9)
    n = 600
    outer = random_intervals(B, n, 3)
    with B.BriskHip(31, 11, 11) as ix:
        d_outer = to_device(outer)

        def inner_for(index, p_drop=0.25):
            rows = []
            for r in index:
                L = int(outer[r]["len"])
                a = rng.randint(0, L - 1)
                rows.append((rng.randint(0, L), 0) if rng.random() < p_drop else (a, rng.randint(1, L - a)))
            return iv_array(B, rows)

        def run(inner, index, n_reads=n):
            d_out = filled_intervals(n_reads)
            d_arg0, d_arg1 = to_device(inner), to_device(np.array(index, np.uint64))   # (held until the call returns)
            ix.compose_intervals(d_outer.data_ptr(), n_reads, d_arg0.data_ptr(), d_arg1.data_ptr(), len(index), d_out.data_ptr())
            got, clean = host_intervals(B, d_out, n_reads)
            assert clean
            return got

        kept = [r for r in range(n) if outer[r]["len"]]           # an index with gaps: what extract_packed writes
        assert 20 < len(kept) < n - 20
        inner = inner_for(kept)
        want = B.compose_intervals(outer, inner, kept)
        assert (want["len"] > 0).sum() >= 20 and (inner["len"] == 0).sum() >= 20
        assert np.array_equal(run(inner, kept), want)
        assert not run(inner[:0], [])["len"].any()                # n_kept 0
        one = [kept[len(kept) // 2]]                               # n_kept 1
        i1 = inner_for(one, 0)
        assert np.array_equal(run(i1, one), B.compose_intervals(outer, i1, one))
        # n_kept == n_reads: an outer cut that keeps everything
        full = outer.copy()
        full["len"] = np.maximum(full["len"], 1)
        d_full = to_device(full)
        rows = [(a, rng.randint(0, int(full[r]["len"]) - a)) for r in range(n) for a in [rng.randint(0, int(full[r]["len"]))]]
        i_all = iv_array(B, rows)
        d_out = filled_intervals(n)
        d_arg0, d_arg1 = to_device(i_all), to_device(np.arange(n, dtype=np.uint64))   # (held until the call returns)
        ix.compose_intervals(d_full.data_ptr(), n, d_arg0.data_ptr(), d_arg1.data_ptr(), n, d_out.data_ptr())
        assert np.array_equal(host_intervals(B, d_out, n)[0], B.compose_intervals(full, i_all, np.arange(n)))

        def refused(inner, index, word):
            d_out = filled_intervals(n)
            with pytest.raises(B.BriskHipError) as e:
                d_arg0, d_arg1 = to_device(inner), to_device(np.array(index, np.uint64))   # (held until the call returns)
                ix.compose_intervals(d_outer.data_ptr(), n, d_arg0.data_ptr(), d_arg1.data_ptr(), len(index), d_out.data_ptr())
            assert e.value.code == EINVAL and word in str(e.value), str(e.value)
            assert host_intervals(B, d_out, 0)[1], "a refused call wrote to its output"
            with pytest.raises(ValueError):
                B.compose_intervals(outer, inner, index)

        bad = inner.copy()
        js = [j for j in range(len(kept)) if inner[j]["len"]]
        for j in (js[40], js[7]):                                  # inner leaves outer, twice: the first is named
            bad[j]["len"] = outer[kept[j]]["len"] - bad[j]["start"] + 1
        refused(bad, kept, "row %d:" % js[7])
        far = list(kept)
        far[-1] = n                                                # the index leaves the table
        refused(inner, far, "row %d:" % (len(kept) - 1))
        swapped = list(kept)
        swapped[5], swapped[6] = swapped[6], swapped[5]
        refused(inner, swapped, "ascend")


# ---- extract_pairs_packed ---------------------------------------------------------------------------------------------------------
def check_pairs_extract(B, ix, reads, intervals, singles=True, cap_pairs=None, cap_singles=None):
    """one call against extract_reference over split_pairs' two tables, word for word; returns the counts"""
    n = len(reads)
    d_packed, d_starts, words, starts = device_reads(reads)
    iv_p, iv_s, counts = B.split_pairs(intervals)
    want = [extract_reference(words, starts, t) for t in (iv_p, iv_s)]
    outs = [OutBuffers(n, len(words) if c is None else c) for c in (cap_pairs, cap_singles)]
    args = [(o.packed.data_ptr(), o.cap, o.starts.data_ptr(), o.index.data_ptr()) for o in outs]
    d_arg0 = to_device(intervals)   # (held until the call returns)
    got_counts = ix.extract_pairs_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_arg0.data_ptr(), args[0], args[1] if singles else None)
    assert got_counts == counts, (got_counts, counts)
    assert counts["n_pairs_in"] == counts["n_pairs_kept"] + counts["n_single_first"] + counts["n_single_second"] + counts["n_pairs_dropped"] == n // 2
    for which, (o, (w_words, w_starts, w_index, w_n, w_nts)) in enumerate(zip(outs, want)):
        if which == 1 and not singles:
            assert o.untouched()
            continue
        got, got_starts, got_index = o.host()
        assert np.array_equal(got[:len(w_words)], w_words), which   # the used words, the zero bits that end the last one, the two zero words after
        assert (got[len(w_words):] == FILL).all(), which             # and nothing else
        assert np.array_equal(got_starts[:w_n + 1], w_starts) and (got_starts[w_n + 1:] == ONES).all(), which
        assert np.array_equal(got_index[:w_n], w_index) and (got_index[w_n:] == ONES).all(), which
        assert w_nts == counts["n_nts_pairs" if which == 0 else "n_nts_singles"]
        if which == 0:
            assert w_n == 2 * counts["n_pairs_kept"] and np.array_equal(got_index[0:w_n:2] + np.uint64(1), got_index[1:w_n:2]) and not (got_index[0:w_n:2] % np.uint64(2)).any()
    return counts


def test_extract_pairs_against_the_numpy_reference(B):
    rng = random.Random(1616)
    reads, ivs = gather_case(rng)
    if len(reads) % 2:
        reads, ivs = reads[:-1], ivs[:-1]
    intervals = iv_array(B, ivs)
    assert {(s % 16, n % 16) for s, n in ivs if n} == {(a, b) for a in range(16) for b in range(16)}
    four_states(B, intervals)
    with B.BriskHip(31, 15, 14) as ix:
        c = check_pairs_extract(B, ix, reads, intervals)
        assert c["n_nts_pairs"] > 256 * 16                           # more than one block of output words
        check_pairs_extract(B, ix, reads, intervals, singles=False)  # singles counted and dropped: the pairs stream is the same, the counts are whole
        check_pairs_extract(B, ix, reads, intervals, cap_pairs=(c["n_nts_pairs"] + 15) // 16 + 2, cap_singles=(c["n_nts_singles"] + 15) // 16 + 2)  # exactly the room
        whole = iv_array(B, [(0, len(r)) for r in reads])
        assert check_pairs_extract(B, ix, reads, whole)["n_pairs_kept"] == len(reads) // 2                     # all pairs intact: the stream itself
        assert check_pairs_extract(B, ix, reads, iv_array(B, [(0, 0)] * len(reads)))["n_pairs_dropped"] == len(reads) // 2
        only = whole.copy()
        only["len"][np.arange(len(reads)) % 4 == 0] = 0              # mate 1 of every even pair gone,
        only["len"][np.arange(len(reads)) % 4 == 3] = 0              # mate 2 of every odd one: singles only
        c = check_pairs_extract(B, ix, reads, only)
        assert c["n_pairs_kept"] == c["n_pairs_dropped"] == 0 and c["n_single_first"] > 0 and c["n_single_second"] > 0
        assert check_pairs_extract(B, ix, [], iv_array(B, []))["n_pairs_in"] == 0
        assert check_pairs_extract(B, ix, ["ACGTT", "GGA"], iv_array(B, [(1, 3), (0, 3)]))["n_nts_pairs"] == 6


def test_extract_pairs_across_blocks(B):
    """2 x 4100 reads of at most 40 nt: pairs sit across k_extract_block's blocks of 4096 reads and its lanes of 16"""
    rng = random.Random(4100)
    n = 2 * 4100
    reads = ["".join(rng.choice("ACGT") for _ in range(rng.randint(1, 40))) for _ in range(n)]
    rows = []
    for r in reads:
        if rng.random() < 0.3:
            rows.append((rng.randint(0, len(r)), 0))
        else:
            a = rng.randrange(len(r))
            rows.append((a, rng.randint(1, len(r) - a)))
    intervals = iv_array(B, rows)
    four_states(B, intervals)
    for r in (4094, 4095, 4096, 4097, 15, 16, 17):                   # kept on both sides of the boundaries
        intervals[r] = (0, len(reads[r]))
    with B.BriskHip(31, 15, 14) as ix:
        check_pairs_extract(B, ix, reads, intervals)


def test_extract_pairs_refusals(B):
    rng = random.Random(3)
    n = 600
    reads = ["".join(rng.choice("ACGT") for _ in range(rng.randint(20, 120))) for _ in range(n)]
    good = iv_array(B, [(2, len(r) - 5) if rng.random() < 0.5 else (0, 0) for r in reads])
    c = four_states(B, good)
    need_p, need_s = (c["n_nts_pairs"] + 15) // 16 + 2, (c["n_nts_singles"] + 15) // 16 + 2
    with B.BriskHip(31, 15, 14) as ix:
        d_packed, d_starts, words, _ = device_reads(reads)

        def call(intervals, cap_p, cap_s, n_reads=n):
            outs = [OutBuffers(n, cap_p), OutBuffers(n, cap_s)]
            args = [(o.packed.data_ptr(), o.cap, o.starts.data_ptr(), o.index.data_ptr()) for o in outs]
            d_arg0 = to_device(intervals)   # (held until the call returns)
            got = ix.extract_pairs_packed(d_packed.data_ptr(), d_starts.data_ptr(), n_reads, d_arg0.data_ptr(), args[0], args[1], raise_on_capacity=False)
            err = ix.L.brisk_hip_last_error(ix.h).decode()
            return got, err, outs

        # room: one word too few on the pairs side, then on the singles side -- nothing written to either, the counts are whole
        for cap_p, cap_s, word in ((need_p - 1, need_s, "pairs"), (need_p, need_s - 1, "singles")):
            got, err, outs = call(good, cap_p, cap_s)
            assert got.pop("rc") == ECAPACITY and got == c and word in err, (got, err)
            assert outs[0].untouched() and outs[1].untouched(), "a refused call wrote to an output"
        assert check_pairs_extract(B, ix, reads, good, cap_pairs=need_p, cap_singles=need_s) == c   # the repeat with room
        # an interval beyond its read, in two reads: the first is named, nothing written
        bad = good.copy()
        bad[211] = (0, len(reads[211]) + 1)
        bad[37] = (len(reads[37]) - 2, 3)
        for intervals, n_reads, word in ((bad, n, "read 37 "), (good, n - 1, "odd")):
            outs = [OutBuffers(n, len(words)), OutBuffers(n, len(words))]
            args = [(o.packed.data_ptr(), o.cap, o.starts.data_ptr(), o.index.data_ptr()) for o in outs]
            with pytest.raises(B.BriskHipError) as e:
                d_arg0 = to_device(intervals)   # (held until the call returns)
                ix.extract_pairs_packed(d_packed.data_ptr(), d_starts.data_ptr(), n_reads, d_arg0.data_ptr(), args[0], args[1])
            assert e.value.code == EINVAL and word in str(e.value), str(e.value)
            assert outs[0].untouched() and outs[1].untouched()
        # a read table that does not ascend
        bad_starts = np.array(device_reads(reads)[3])
        bad_starts[3], bad_starts[4] = bad_starts[4], bad_starts[3]
        outs = [OutBuffers(n, len(words)), OutBuffers(n, len(words))]
        args = [(o.packed.data_ptr(), o.cap, o.starts.data_ptr(), o.index.data_ptr()) for o in outs]
        with pytest.raises(B.BriskHipError) as e:
            d_arg0, d_arg1 = to_device(bad_starts), to_device(good)   # (held until the call returns)
            ix.extract_pairs_packed(d_packed.data_ptr(), d_arg0.data_ptr(), n, d_arg1.data_ptr(), args[0], args[1])
        assert e.value.code == EINVAL and "ascend" in str(e.value) and outs[0].untouched() and outs[1].untouched()
        # null pointers; a singles output given in part
        pc = B.hipapi._PairCounts()
        d_iv = to_device(good)
        full = [ix.h, d_packed.data_ptr(), d_starts.data_ptr(), n, d_iv.data_ptr(), *args[0], *args[1], C.byref(pc)]
        for hole in (0, 1, 2, 4, 5, 7, 9, 11, 13):
            a = list(full)
            a[hole] = None
            assert ix.L.brisk_hip_extract_pairs_packed(*a) == EINVAL, hole
        assert outs[0].untouched() and outs[1].untouched()


# ---- trim_pairs_packed / trim_pairs_reads -----------------------------------------------------------------------------------------
def whole_reads(B, prof, k, min_len):
    """what a mate is when kept uncut: [0, n_kmers + k - 1), dropped below max(min_len, k) nucleotides"""
    length = np.where(prof["n_kmers"] > 0, prof["n_kmers"].astype(np.int64) + k - 1, 0)
    out = np.zeros(len(prof), B.READ_INTERVAL_DTYPE)
    out["len"] = np.where(length >= max(min_len, k), length, 0)
    return out


@pytest.mark.parametrize("k,m,b", E2E_GEOMETRIES)
def test_trim_pairs_against_the_host_route(B, k, m, b):
    seqs = error_reads(k, 800, seed=21)
    random.Random(21).shuffle(seqs)               # (neighbours in the generator's order share their fate: mates should not)
    seqs = seqs[:len(seqs) // 2 * 2]
    n = len(seqs)
    assert n >= 600
    with B.BriskHip(k, m, b) as ix, B.BriskHip(k, m, b, max_batch_reads=97) as small:
        for h in (ix, small):
            h.insert_reads(seqs[:2 * n // 3])     # (the other reads' errors are k-mers the index does not hold)
        prof = B.profile_from_slots(*ix.get_kmers(seqs), 2)
        # rules that tell the reads apart, chosen from the numpy side: the threshold that keeps closest to half of the reads
        runs = B.intervals_from_profile(prof, k, B.select_rule("solid_run"))["len"].astype(np.int64)
        medians = prof["median"].astype(np.int64)
        min_len = min(np.unique(runs[runs > 0]), key=lambda t: abs((runs >= t).mean() - 0.5))
        hi = min(np.unique(medians), key=lambda t: abs(((medians <= t) & (prof["n_kmers"] > 0)).mean() - 0.5))
        rules = {"solid_run": B.select_rule("solid_run", min_len=int(min_len)), "median": B.select_rule("median", lo=0, hi=int(hi))}
        d_packed, d_starts, words, starts = device_reads(seqs)
        for name, rule in rules.items():
            each = B.intervals_from_profile(prof, k, rule)
            whole = whole_reads(B, prof, k, rule.min_len)
            four_states(B, each)
            for mode in ("each", "all", "any"):
                final = B.pair_intervals(each, whole, mode)
                iv_p, iv_s, counts = B.split_pairs(final)
                want = [extract_reference(words, starts, t) for t in (iv_p, iv_s)]
                for h in (ix, small):             # several internal batches, a batch boundary inside a pair: the same answer
                    got_iv, got_counts = h.trim_pairs(seqs, None, 2, rule, mode)
                    assert np.array_equal(got_iv, final), (name, mode, int(np.nonzero(got_iv != final)[0][0]))
                    assert got_counts == counts, (name, mode)
                    outs = [OutBuffers(n, len(words)), OutBuffers(n, len(words))]
                    args = [(o.packed.data_ptr(), o.cap, o.starts.data_ptr(), o.index.data_ptr()) for o in outs]
                    assert h.trim_pairs_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, args[0], args[1], 2, rule, mode) == counts, (name, mode)
                    for o, (w_words, w_starts, w_index, w_n, _) in zip(outs, want):
                        got, got_starts, got_index = o.host()
                        assert np.array_equal(got[:len(w_words)], w_words) and (got[len(w_words):] == FILL).all(), (name, mode)
                        assert np.array_equal(got_starts[:w_n + 1], w_starts) and np.array_equal(got_index[:w_n], w_index), (name, mode)
                if mode == "any":
                    assert (final["len"] > each["len"]).any(), "no mate was restored whole"
        got_iv, got_counts = ix.trim_pairs(seqs[0::2], seqs[1::2], 2, rules["median"], "all")   # two lists: interleaved by the wrapper
        assert np.array_equal(got_iv, B.pair_intervals(B.intervals_from_profile(prof, k, rules["median"]), None, "all"))
        with pytest.raises(ValueError):
            ix.trim_pairs(seqs[:3])
        with pytest.raises(ValueError):
            ix.trim_pairs(seqs[:4], seqs[:3])


def test_trim_pairs_refusals(B):
    rng = random.Random(5)
    reads = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(20)]
    d_packed, d_starts, words, _ = device_reads(reads)
    for kw, word in ((dict(entry_ids=True), "entry-id"), (dict(n_owners=2, owner_rank=0), "sharded")):
        with B.BriskHip(31, 15, 14, **kw) as ix:
            outs = [OutBuffers(len(reads), len(words)), OutBuffers(len(reads), len(words))]
            args = [(o.packed.data_ptr(), o.cap, o.starts.data_ptr(), o.index.data_ptr()) for o in outs]
            with pytest.raises(B.BriskHipError) as e:
                ix.trim_pairs_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), args[0], args[1])
            assert e.value.code == EINVAL and word in str(e.value) and outs[0].untouched() and outs[1].untouched()
            with pytest.raises(B.BriskHipError) as e:
                ix.trim_pairs(reads)
            assert e.value.code == EINVAL and word in str(e.value)
            whole = iv_array(B, [(0, 150)] * len(reads))
            assert check_pairs_extract(B, ix, reads, whole)["n_pairs_kept"] == 10   # the split needs no index
    with B.BriskHip(31, 15, 14) as ix:
        pc = B.hipapi._PairCounts()
        out = np.zeros(len(reads), B.READ_INTERVAL_DTYPE)
        flat = np.frombuffer("".join(reads).encode(), np.uint8).copy()
        offs = np.arange(len(reads) + 1, dtype=np.uint64) * np.uint64(150)
        rule = B.select_rule("solid_run")
        assert ix.L.brisk_hip_trim_pairs_reads(ix.h, flat, offs, len(reads), 2, C.byref(rule), 3, out, C.byref(pc)) == EINVAL
        assert ix.L.brisk_hip_trim_pairs_reads(ix.h, flat, offs, len(reads) - 1, 2, C.byref(rule), 0, out, C.byref(pc)) == EINVAL
        assert ix.L.brisk_hip_trim_pairs_reads(ix.h, flat, offs, len(reads), 2, C.byref(B.select_rule(3)), 0, out, C.byref(pc)) == EINVAL
        assert ix.L.brisk_hip_trim_pairs_reads(ix.h, flat, offs, len(reads), 2, C.byref(rule), 0, out, C.byref(pc)) == 0


# ---- clean_pairs ------------------------------------------------------------------------------------------------------------------
def raw_pairs(k, n=600, seed=31, n_src=None, junk=None):
    """raw reads of 30..200 bytes cut from error-bearing reads over a small genome (from the first n_src of them): N, lower case, other
    bytes (of `junk`; by default any byte that is no base, line ends among them), qualities; reads with no, one and several
    fragments, and an empty read"""
    rng = random.Random(seed)
    src = [s for s in error_reads(k, 1200, seed=seed) if len(s) >= 100][:n_src]
    seqs, quals = [], []
    for i in range(n):
        s = bytearray(src[i % len(src)][:rng.randint(30, 200)].encode())
        kind = rng.random()
        if i == 5:
            s = bytearray()
        elif kind < 0.35:                      # no fragment: an N every few bytes
            for p in range(rng.randint(0, k - 2), len(s), k - 1):
                s[p] = ord("N")
        elif kind < 0.65:                      # several fragments
            for _ in range(rng.randint(1, 3)):
                p = rng.randrange(len(s))
                s[p:p + rng.randint(1, 3)] = invalid_run(rng, 1) if junk is None else bytes([rng.choice(junk)])
        if kind > 0.7:
            a = rng.randrange(max(len(s), 1))
            s[a:a + 20] = bytes(s[a:a + 20]).lower()
        q = bytearray(rng.choice(b"5:?DI") for _ in range(len(s)))
        if rng.random() < 0.3 and len(s) > 10:
            p = rng.randrange(len(s))
            q[p] = ord("#")                    # Phred 2
        seqs.append(bytes(s))
        quals.append(bytes(q))
    return seqs, quals


def clean_route(B, ix, seqs, quals, k, intake, rule, solid_min, mode):
    """fragments_from_reads -> intervals_from_fragments; with a rule the host route over the fragment strings, composed back"""
    frags, stats = B.fragments_from_reads(seqs, quals, k, intake)
    iv1 = B.intervals_from_fragments(frags, len(seqs))
    each = iv1
    if rule is not None:
        index = np.nonzero(iv1["len"] > 0)[0]
        strings = [seqs[r][int(iv1[r]["start"]):int(iv1[r]["start"]) + int(iv1[r]["len"])] for r in index]
        inner = B.intervals_from_profile(B.profile_from_slots(*ix.get_kmers(strings), solid_min), k, rule)
        each = B.compose_intervals(iv1, inner, index)
    return B.pair_intervals(each, iv1, mode), each, iv1, stats


@pytest.mark.parametrize("with_rule", (False, True))
def test_clean_pairs(B, with_rule, monkeypatch):
    k, m, b = 31, 11, 11
    seqs, quals = raw_pairs(k)
    n = len(seqs)
    intake = B.intake_rule(min_qual=10)
    flat = np.frombuffer(b"".join(seqs), np.uint8).copy()
    qflat = np.frombuffer(b"".join(quals), np.uint8).copy()
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    words, starts = pack_reads(seqs)
    with B.BriskHip(k, m, b) as ix:
        rule = None
        if with_rule:
            for _ in range(2):                 # (counted twice: a k-mer that the first two thirds hold is solid)
                ix.insert_raw(seqs[:2 * n // 3], quals[:2 * n // 3], intake)
            rule = B.select_rule("solid_run", min_len=40)
        frags, _ = B.fragments_from_reads(seqs, quals, k, intake)
        per_read = np.bincount(frags["read"].astype(np.int64), minlength=n)
        assert (per_read == 0).sum() >= 20 and (per_read == 1).sum() >= 20 and (per_read >= 2).sum() >= 20 and len(seqs[5]) == 0
        d_bases, d_quals, d_offs = to_device(flat), to_device(qflat), to_device(offs)
        for mode in ("each", "all", "any"):
            final, each, iv1, stats = clean_route(B, ix, seqs, quals, k, intake, rule, 2, mode)
            four_states(B, each)
            if with_rule:
                assert ((each["len"] > 0) & (each["len"] < iv1["len"])).sum() >= 20, "the rule cut nothing"
            for r in np.nonzero(final["len"])[0]:
                s = seqs[r][int(final[r]["start"]):int(final[r]["start"]) + int(final[r]["len"])]
                assert len(s) == final[r]["len"] and re.fullmatch(b"[ACGTacgt]+", s)
            iv_p, iv_s, counts = B.split_pairs(final)
            want = [extract_reference(words, starts, t) for t in (iv_p, iv_s)]
            outs = [OutBuffers(n, len(words)), OutBuffers(n, len(words))]
            args = [(o.packed.data_ptr(), o.cap, o.starts.data_ptr(), o.index.data_ptr()) for o in outs]
            d_iv = filled_intervals(n)
            got_counts, got_stats = ix.clean_pairs_ascii(d_bases.data_ptr(), d_quals.data_ptr(), d_offs.data_ptr(), n, intake, args[0], args[1], rule, 2, mode, d_iv.data_ptr())
            assert got_counts == counts and got_stats == stats, (mode, got_counts, counts)
            got_iv, clean = host_intervals(B, d_iv, n)
            assert np.array_equal(got_iv, final) and clean, (mode, int(np.nonzero(got_iv != final)[0][0]) if not np.array_equal(got_iv, final) else -1)
            for o, (w_words, w_starts, w_index, w_n, _) in zip(outs, want):
                got, got_starts, got_index = o.host()
                assert np.array_equal(got[:len(w_words)], w_words) and (got[len(w_words):] == FILL).all(), mode
                assert np.array_equal(got_starts[:w_n + 1], w_starts) and np.array_equal(got_index[:w_n], w_index), mode
            # the host call, and the two-list form
            got_iv, got_counts, got_stats = ix.clean_pairs(seqs, None, quals, None, intake, rule, 2, mode)
            assert np.array_equal(got_iv, final) and got_counts == counts and got_stats == stats, mode
        got_iv2, _, _ = ix.clean_pairs(seqs[0::2], seqs[1::2], quals[0::2], quals[1::2], intake, rule, 2, "any")
        assert np.array_equal(got_iv2, final)
        # a table that begins past 0: the reads from the 100th on, addressed by their own offsets
        first = next(r for r in range(100, n, 2) if offs[r] % 16)   # (the bytes are packed from a byte that is not 16-byte aligned)
        final_sub = clean_route(B, ix, seqs[first:], quals[first:], k, intake, rule, 2, "each")[0]
        d_iv = filled_intervals(n - first)
        outs = [OutBuffers(n, len(words)), OutBuffers(n, len(words))]
        args = [(o.packed.data_ptr(), o.cap, o.starts.data_ptr(), o.index.data_ptr()) for o in outs]
        ix.clean_pairs_ascii(d_bases.data_ptr(), d_quals.data_ptr(), d_offs.data_ptr() + 8 * first, n - first, intake, args[0], args[1], rule, 2, "each", d_iv.data_ptr())
        assert np.array_equal(host_intervals(B, d_iv, n - first)[0], final_sub)
        p_sub = extract_reference(*pack_reads(seqs[first:]), B.split_pairs(final_sub)[0])
        assert np.array_equal(outs[0].host()[0][:len(p_sub[0])], p_sub[0])
        # room and refusals
        c = B.split_pairs(final)[2]
        outs = [OutBuffers(n, (c["n_nts_pairs"] + 15) // 16 + 1), OutBuffers(n, len(words))]
        args = [(o.packed.data_ptr(), o.cap, o.starts.data_ptr(), o.index.data_ptr()) for o in outs]
        d_iv = filled_intervals(n)
        got_counts, _ = ix.clean_pairs_ascii(d_bases.data_ptr(), d_quals.data_ptr(), d_offs.data_ptr(), n, intake, args[0], args[1], rule, 2, "any", d_iv.data_ptr(), raise_on_capacity=False)
        assert got_counts.pop("rc") == ECAPACITY and got_counts == c and outs[0].untouched() and outs[1].untouched() and host_intervals(B, d_iv, 0)[1]
        with pytest.raises(B.BriskHipError) as e:
            ix.clean_pairs_ascii(d_bases.data_ptr(), d_quals.data_ptr(), d_offs.data_ptr(), n - 1, intake, args[0], args[1], rule)
        assert e.value.code == EINVAL and "odd" in str(e.value) and outs[0].untouched() and outs[1].untouched()
    # pieces of whole pairs: a piece size that cuts the call into many pieces (read when the handle is created)
    monkeypatch.setenv("BRISK_INTAKE_PIECE", "700")
    with B.BriskHip(k, m, b) as ix:
        for _ in range(2 if with_rule else 0):
            ix.insert_raw(seqs[:2 * n // 3], quals[:2 * n // 3], intake)
        got_iv, got_counts, got_stats = ix.clean_pairs(seqs, None, quals, None, intake, rule, 2, "any")
        assert np.array_equal(got_iv, final) and got_counts == B.split_pairs(final)[2] and got_stats == stats
    if with_rule:
        for kw, word in ((dict(entry_ids=True), "entry-id"), (dict(n_owners=2, owner_rank=0), "sharded")):
            with B.BriskHip(31, 15, 14, **kw) as ix:
                with pytest.raises(B.BriskHipError) as e:
                    ix.clean_pairs(seqs[:10], None, quals[:10], None, intake, rule)
                assert e.value.code == EINVAL and word in str(e.value)
                assert np.array_equal(ix.clean_pairs(seqs[:10], None, quals[:10], None, intake, None)[0], clean_route(B, None, seqs[:10], quals[:10], 31, intake, None, 2, "each")[0])


# ---- brisk_count --paired ---------------------------------------------------------------------------------------------------------
def fasta_text(seqs):
    return "".join(">r%d\n%s\n" % (i, "\n".join(s[j:j + 70] for j in range(0, len(s), 70))) for i, s in enumerate(seqs))


def fastq_text(seqs, quals):
    return "".join("@r%d\n%s\n+\n%s\n" % (i, s.decode("latin-1"), q.decode("latin-1")) for i, (s, q) in enumerate(zip(seqs, quals)))


def expected_files(seqs, final):
    """the three files of --paired --extract from the interleaved reads and their final intervals"""
    out = ["", "", ""]
    for p in range(len(seqs) // 2):
        both = final[2 * p]["len"] and final[2 * p + 1]["len"]
        for mate in (0, 1):
            v = final[2 * p + mate]
            if v["len"]:
                s = seqs[2 * p + mate][int(v["start"]):int(v["start"]) + int(v["len"])]
                out[mate if both else 2] += ">%d/%d %d %d\n%s\n" % (p, mate + 1, v["start"], v["len"], s if isinstance(s, str) else s.decode("latin-1"))
    return out


def test_brisk_count_paired(B, tmp_path):
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe):
        B.build_apps()
    k, m, b = 31, 11, 11
    seqs = [s for s in error_reads(k, 1400, seed=41) if len(s) >= 20]
    random.Random(41).shuffle(seqs)               # (neighbours in the generator's order share their fate: mates should not)
    seqs = seqs[:len(seqs) // 2 * 2]
    n = len(seqs)

    def run(args, ok=True):
        p = subprocess.run([exe, "--bulk"] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
        assert (p.returncode == 0) == ok, (p.returncode, p.stderr[-2000:])
        return p

    def files(prefix):
        return [open("%s.%s.fa" % (prefix, x)).read() for x in ("1", "2", "s")]

    inter, one, two, lone = (str(tmp_path / x) for x in ("inter.fa", "one.fa", "two.fa", "all.fa"))
    open(inter, "w").write(fasta_text(seqs))
    open(one, "w").write(fasta_text(seqs[0::2]))
    open(two, "w").write(fasta_text(seqs[1::2]))
    open(lone, "w").write(fasta_text(seqs[0::2] + seqs[1::2]))
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(seqs)
        # a minimum length that tells the reads apart, chosen from the numpy side: the one that keeps closest to half of them
        prof = B.profile_from_slots(*ix.get_kmers(seqs), 2)
        runs = B.intervals_from_profile(prof, k, B.select_rule("solid_run"))["len"].astype(np.int64)
        min_len = int(min(np.unique(runs[runs > 0]), key=lambda t: abs((runs >= t).mean() - 0.5)))
        rule = B.select_rule("solid_run", min_len=min_len)
        each = B.intervals_from_profile(prof, k, rule)
        four_states(B, each)
        for mode in ("each", "any"):
            final, counts = ix.trim_pairs(seqs, None, 2, rule, mode)
            assert np.array_equal(final, B.pair_intervals(each, whole_reads(B, prof, k, min_len), mode)), mode
            want = expected_files(seqs, final)
            pre = str(tmp_path / ("i_" + mode))
            p = run([inter, k, m, b, "--paired", "--pair-mode", mode, "--extract", pre, "--rule", "trim", "--min-len", min_len, "--save", pre + ".snap"])
            assert files(pre) == want, mode
            line = [x for x in p.stderr.splitlines() if x.startswith("pairs ")]
            assert len(line) == 1 and all("%s=%d" % (f, counts[f]) in line[0] for f in B.PAIR_COUNTS_FIELDS[:7]), p.stderr
            pre2 = str(tmp_path / ("m_" + mode))
            run([one, k, m, b, "--paired", "--mate", two, "--pair-mode", mode, "--extract", pre2, "--min-len", min_len, "--save", pre2 + ".snap"])
            assert files(pre2) == want, mode
        # pairing never changes the index: the digest of the paired runs is that of the same reads counted unpaired
        run([lone, k, m, b, "--save", str(tmp_path / "lone.snap")])
        digest = B.snapshot_info(str(tmp_path / "lone.snap"))["checksum"]
        assert digest[0] > 0 and digest == B.snapshot_info(pre + ".snap")["checksum"] == B.snapshot_info(pre2 + ".snap")["checksum"] == ix.checksum()
    # FASTQ: two files, cut by quality on the device, then by abundance
    rseqs, rquals = raw_pairs(k, 1200, seed=43, n_src=400, junk=b"NnRY-.@")   # (no line ends inside a FASTQ line)
    q1, q2 = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    open(q1, "w", encoding="latin-1").write(fastq_text(rseqs[0::2], rquals[0::2]))
    open(q2, "w", encoding="latin-1").write(fastq_text(rseqs[1::2], rquals[1::2]))
    intake = B.intake_rule(min_qual=10)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_raw(rseqs, rquals, intake)
        final, counts, _ = ix.clean_pairs(rseqs, None, rquals, None, intake, B.select_rule("solid_run"), 2, "each")
        want_final = clean_route(B, ix, rseqs, rquals, k, intake, B.select_rule("solid_run"), 2, "each")[0]
        four_states(B, want_final)
        assert np.array_equal(final, want_final)
        pre = str(tmp_path / "q")
        p = run([q1, k, m, b, "--paired", "--mate", q2, "--min-qual", 10, "--extract", pre, "--save", pre + ".snap"])
        got = [open("%s.%s.fa" % (pre, x), encoding="latin-1").read() for x in ("1", "2", "s")]
        assert got == expected_files(rseqs, final)
        assert "n_pairs_kept=%d " % counts["n_pairs_kept"] in p.stderr
        assert B.snapshot_info(pre + ".snap")["checksum"] == ix.checksum()
    # refusals: exit status 2 with a message
    open(str(tmp_path / "odd.fa"), "w").write(fasta_text(seqs[:7]))
    open(str(tmp_path / "short.fa"), "w").write(fasta_text(seqs[1:n - 1:2]))
    dirty, never = str(tmp_path / "dirty.fa"), str(tmp_path / "never.snap")
    j = next(i for i in range(1, 20, 2) if len(seqs[i]) >= 60)
    open(dirty, "w").write(fasta_text(seqs[:j] + [seqs[j][:40] + "N" + seqs[j][41:]] + seqs[j + 1:20]))
    p = run([dirty, k, m, b, "--paired", "--extract", str(tmp_path / "d"), "--save", never], ok=False)
    assert p.returncode == 2 and "mate 2 of pair %d " % (j // 2) in p.stderr and not os.path.exists(never) and not os.path.exists(str(tmp_path / "d.1.fa")), p.stderr  # refused before anything is counted or written
    for args, word in (([str(tmp_path / "odd.fa"), k, m, b, "--paired"], "odd"), ([one, k, m, b, "--paired", "--mate", str(tmp_path / "short.fa")], "--mate"),
                       ([q1, k, m, b, "--extract", str(tmp_path / "x.fa")], "FASTQ"), ([one, k, m, b, "--mate", two], "--paired"),
                       ([inter, k, m, b, "--paired", "--pair-mode", "some"], "--pair-mode"), ([one, k, m, b, "--paired", "--mate", q2], "both")):
        p = run(args, ok=False)
        assert p.returncode == 2 and word in p.stderr, (args, p.stderr)
