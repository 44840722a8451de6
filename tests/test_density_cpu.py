"""CPU: the oracle's threaded entry points, its C digest and bucket filter, and the dense read generator -- the tools
tests/test_density_parity.py compares the HIP path with at 10^5 .. 10^6 reads.  Everything here is integer work: bit-exact."""
import numpy as np
import pytest

import oracle
from density_reads import (as_strings, concat_reads, cut_at_invalid, dense_reads, entry_diff, poly_a_reads, substitute,
                           take_reads)

GEOMETRIES = [(63, 21, 14), (31, 15, 14), (31, 11, 11)]


def _mixed_reads(k, n=50_000, seed=5):
    """>= 50 k reads with everything the generator has: errors, N cuts, pieces shorter than k, repeats, tandem reads, lower
    case; and one read 300 times, so that a count wraps."""
    flat, offs = dense_reads(n, k, 400_000, seed, e=0.01, p_n=0.01, repeat_len=500, repeat_copies=20, n_special=300)
    wrap = take_reads(flat, offs, np.full(300, 17))
    return concat_reads([(flat, offs), wrap])


def _sorted_entries(dump):
    lo, hi, idx, cnt = dump
    order = np.lexsort((idx, lo, hi))
    return lo[order], hi[order], idx[order], cnt[order]


def _index(O, k, m, b, flat, offs, threads=1, mt=False, bucket_range=None):
    h = O.index_new(k, m, b)
    if bucket_range:
        O.index_set_bucket_range(h, *bucket_range)
    if mt:
        O.index_insert_reads_mt(h, flat, offs, threads)
    else:
        O.index_insert_reads(h, flat, offs, threads=threads)
    return h


@pytest.mark.parametrize("k,m,b", GEOMETRIES)
def test_threaded_insert_and_query_equal_the_single_threaded_ones(O, k, m, b):
    flat, offs = _mixed_reads(k)
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    assert len(lens) >= 50_000 and (lens < k).sum() > 100 and (lens >= k).sum() > 40_000
    h1 = _index(O, k, m, b, flat, offs)
    want = _sorted_entries(O.index_dump(h1))
    assert len(want[0]) > 100_000
    assert int(want[3].sum(dtype=np.int64)) < int(np.maximum(lens - k + 1, 0).sum())  # read 17 went in 301 times: counts wrapped
    want_stats = O.index_stats(h1)
    want_skm = O.lib.bo_index_nb_skm_seen(C_void(h1))
    qf, qo = concat_reads([take_reads(flat, offs, np.arange(0, 20_000)), poly_a_reads(500, k, 3),
                           dense_reads(3000, k, 50_000, 77, n_special=0)])
    qf = substitute(qf, 0.01, 9)
    want_q = O.index_query_reads(h1, qf, qo)
    assert want_q.sum() > 0
    for threads in (1, 3, 16):
        h = _index(O, k, m, b, flat, offs, threads=threads, mt=True)
        got = _sorted_entries(O.index_dump(h))
        assert all(np.array_equal(a, c) for a, c in zip(got, want)), (threads, entry_diff(got, want, k))
        assert O.index_stats(h) == want_stats, threads
        assert O.lib.bo_index_nb_skm_seen(C_void(h)) == want_skm
        assert O.index_digest(h) == O.index_digest(h1)
        assert np.array_equal(O.index_query_reads(h, qf, qo, threads=threads), want_q), threads
        O.index_free(h)
    # Oracle.index_insert_reads(threads=) is that path
    h = _index(O, k, m, b, flat, offs, threads=4)
    assert O.index_digest(h) == O.index_digest(h1) and O.index_stats(h) == want_stats
    O.index_free(h)
    O.index_free(h1)


def C_void(h):
    import ctypes
    return ctypes.c_void_p(h)


def test_a_count_that_wraps_wraps_the_same_way_over_threads(O):
    s = "ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGGCTAGCTAGCTAGGCTAG"
    flat, offs = oracle.pack_reads([s] * 300 + [s[:40]] * 250 + ["ACG"])
    for threads in (1, 2, 16):
        h = _index(O, 31, 11, 4, flat, offs, threads=threads, mt=True)
        lo, hi, idx, cnt = O.index_dump(h)
        O.index_free(h)
        assert sorted(cnt.tolist()) == sorted([550 % 256] * 10 + [300 % 256] * (len(s) - 40)), threads


def test_c_digest_is_the_python_digest(O):
    flat, offs = dense_reads(60, 31, 5000, 2, n_special=10)
    for k, m, b in GEOMETRIES:
        h = _index(O, k, m, b, flat, offs)
        dump = O.index_dump(h)
        assert 2000 < len(dump[0]) < 20_000
        want = oracle.digest(*dump)
        assert O.index_digest(h) == want
        assert O.digest_entries(*dump) == want
        p = np.random.default_rng(1).permutation(len(dump[0]))
        assert O.digest_entries(*(a[p] for a in dump)) == want  # order-independent
        O.index_free(h)
    assert O.digest_entries(*(np.zeros(0, t) for t in (np.uint64, np.uint64, np.uint8, np.uint8))) == (0, 0, 0)


@pytest.mark.parametrize("k,m,b", GEOMETRIES)
def test_bucket_filter_is_a_cut_of_the_full_index(O, k, m, b):
    flat, offs = _mixed_reads(k, n=20_000, seed=8)
    full = _index(O, k, m, b, flat, offs, threads=4)
    dump = O.index_dump(full)
    ids = O.bucket_ids(full, dump[0], dump[1], dump[2], threads=3)
    assert np.array_equal(ids, O.bucket_ids(full, dump[0], dump[1], dump[2]))
    n_buckets = 1 << (2 * b)
    assert ids.max() < n_buckets and len(np.unique(ids)) == O.index_stats(full)[1]
    cuts = [0, n_buckets // 3, n_buckets // 3 + n_buckets // 16, n_buckets]  # two ranges and their complement's rest
    seen = 0
    for first, last in zip(cuts[:-1], cuts[1:]):
        for threads in (1, 16):
            h = _index(O, k, m, b, flat, offs, threads=threads, bucket_range=(first, last))
            inside = (ids >= first) & (ids < last)
            want = _sorted_entries(tuple(a[inside] for a in dump))
            got = _sorted_entries(O.index_dump(h))
            assert all(np.array_equal(a, c) for a, c in zip(got, want)), (first, last, entry_diff(got, want, k))
            assert O.index_digest(h) == O.digest_entries(*want)
            assert O.index_stats(h) == (int(inside.sum()), len(np.unique(ids[inside])))
            O.index_free(h)
        seen += int(inside.sum())
    assert seen == len(ids)
    for bad in ((5, 5), (0, n_buckets + 1)):
        with pytest.raises(ValueError):
            O.index_set_bucket_range(full, *bad)
    O.index_free(full)


def test_generator_is_deterministic_and_equals_the_string_path():
    k = 31
    kw = dict(e=0.02, p_n=0.3, repeat_len=200, repeat_copies=3, n_special=40, lower_share=0.2, ragged_share=0.2)
    raw, raw_offs = dense_reads(400, k, 20_000, 11, cut=False, **kw)
    flat, offs = dense_reads(400, k, 20_000, 11, **kw)
    again = dense_reads(400, k, 20_000, 11, **kw)
    assert np.array_equal(flat, again[0]) and np.array_equal(offs, again[1])
    other = dense_reads(400, k, 20_000, 12, **kw)
    assert not np.array_equal(flat[:1000], other[0][:1000])
    records = as_strings(raw, raw_offs)
    assert sum("N" in r for r in records) > 60
    records += ["NNACGTNNacgtN", "N", "ACGNNNNNNNNNNT", "NACGT" * 20, "acgtn" + "ACGT" * 30 + "N", "ACGT" * 10]  # N first, last, alone, dense
    raw, raw_offs = oracle.pack_reads(records)
    flat, offs = concat_reads([(flat, offs), cut_at_invalid(*oracle.pack_reads(records[-6:]))])
    text = "".join(f">r{i}\n" + "".join(r[j:j + 60] + "\n" for j in range(0, len(r), 60)) for i, r in enumerate(records))
    want = oracle.fasta_sequences(text)
    got = as_strings(flat, offs)
    assert any(s != s.upper() for s in got)  # lower case is kept ...
    assert [s.upper() for s in got] == want  # ... and is all that differs from the string path
    assert len(got) > len(records) and min(map(len, got)) < k - 2 and "" not in got
    lens = np.array([len(r) for r in records])
    assert {100, 150, 250} <= set(lens.tolist()) and ((lens >= k - 2) & (lens <= k + 2)).sum() > 20
    assert np.array_equal(cut_at_invalid(flat, offs)[1], offs)  # nothing left to cut


def test_generator_substitution_rate_and_strands():
    g_len, k = 50_000, 31
    clean, offs = dense_reads(2000, k, g_len, 4, e=0.0, p_n=0.0, n_special=0, lower_share=0.0)
    noisy, offs2 = dense_reads(2000, k, g_len, 4, e=0.01, p_n=0.0, n_special=0, lower_share=0.0)
    assert len(clean) == len(noisy)
    # the same reads (the error draw comes after a chunk's positions and strands), about 1 % of the bases substituted
    assert np.array_equal(offs, offs2)
    rate = float((clean != noisy).mean())
    assert 0.008 < rate < 0.012, rate
    from density_reads import random_genome
    genome = bytes(b"ACTG"[c] for c in random_genome(g_len, 4)).decode()
    comp = str.maketrans("ACGT", "TGCA")
    hits = 0
    for r in as_strings(clean, offs)[:200]:
        assert r in genome or r[::-1].translate(comp) in genome
        hits += r in genome
    assert 60 < hits < 140  # both strands


def test_entry_diff_names_what_differs():
    lo = np.array([5, 1, 9, 7], np.uint64)
    hi = np.array([0, 0, 1, 0], np.uint64)
    idx = np.array([2, 3, 4, 5], np.uint8)
    cnt = np.array([1, 2, 3, 4], np.uint8)
    assert entry_diff((lo, hi, idx, cnt), (lo[::-1], hi[::-1], idx[::-1], cnt[::-1]), 33) == ""
    got = (lo[[0, 1, 2]], hi[[0, 1, 2]], idx[[0, 1, 2]], np.array([1, 9, 3], np.uint8))
    want = (lo[[1, 2, 3]], hi[[1, 2, 3]], idx[[1, 2, 3]], cnt[[1, 2, 3]])
    rep = entry_diff(got, want, 33).split("\n")
    a = "A" * 30
    assert rep == ["missing from the index under test: 1", f"  {a}ACG 5 4", "extra in the index under test: 1", f"  {a}ACC 2 1",
                   "present with another count: 1", f"  {a}AAC 3 9 (want 2)"]


@pytest.mark.skipif(not oracle.have_ref(), reason="oracle/_ref/libbrisk_ref.so is not built (needs the reference tree)")
@pytest.mark.parametrize("k,m,b", [(63, 21, 14), (31, 15, 14)])
def test_threaded_restatement_equals_the_reference_build_at_200k_reads(O, k, m, b):
    """The mid-size pin of the restatement: the reference's own sources (oracle/_ref, 16 threads) and the threaded restatement
    on >= 200 k error-bearing reads."""
    R = oracle.Ref()
    flat, offs = dense_reads(200_000, k, 3_000_000, 21, e=0.01, p_n=0.002, repeat_len=800, repeat_copies=30, n_special=300)
    assert len(offs) - 1 >= 200_000
    h = _index(O, k, m, b, flat, offs, threads=16)
    r = R.index_new(k, m, b)
    R.index_insert_reads(r, flat, offs, threads=16)
    got, want = O.index_dump(h), R.index_dump(r)
    assert O.index_stats(h) == R.index_stats(r)
    assert O.digest_entries(*got) == O.digest_entries(*want), entry_diff(got, want, k)
    qf, qo = take_reads(flat, offs, np.arange(0, len(offs) - 1, 40))
    qf = substitute(qf, 0.01, 3)
    assert np.array_equal(O.index_query_reads(h, qf, qo, threads=16), R.index_query_reads(r, qf, qo))
    O.index_free(h)
    R.index_free(r)
