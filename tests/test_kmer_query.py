"""GPU: the per-k-mer get (brisk_hip_get_kmers / _packed) against the oracle.  The expected answer of a slot comes from the
oracle's enumerator run over the whole read: its vectors are consecutive along the read, a vector whose k-mers are the read's
own sits at ascending positions, one whose k-mers are reverse complements at descending ones; each (kmer_s, minimizer_idx) is
then looked up in the oracle's index (0 absent, 0x100 | count present)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle
from test_gpu_parity import SPECIAL, _random_reads

pytestmark = pytest.mark.gpu

GEOMETRIES = [(63, 21, 14), (31, 15, 14), (31, 11, 11), (47, 15, 10)]  # (47, 15, 10): no fast kernel, the generic probe body


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    assert brisk_amd.library_path()
    return brisk_amd


def _codes(s) -> np.ndarray:
    b = s.encode() if isinstance(s, str) else bytes(s)
    return (np.frombuffer(b, np.uint8) >> 1) & 3  # nuc2int (Kmers.cpp:442-444)


def _window_words(codes: np.ndarray, k: int):
    """(lo, hi) of the k-mer at every position, as the oracle encodes them (first nt most significant)"""
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    c = codes.astype(np.uint64)
    nlo = min(k, 32)
    lo = np.zeros(n, np.uint64)
    hi = np.zeros(n, np.uint64)
    for i in range(k):
        col = c[i:i + n]
        if i >= k - nlo:
            lo |= col << np.uint64(2 * (k - 1 - i))
        else:
            hi |= col << np.uint64(2 * (k - nlo - 1 - i))
    return lo, hi


def expected_slots(O, h, read, k: int, m: int):
    """The slots of one read: (values uint16[nk], [(start, end, alternative values)] for vectors whose span is its own reverse
    complement -- both orientations then fit the vector, and which one the enumerator took is not visible in its output)."""
    codes = _codes(read)
    nk = max(len(codes) - k + 1, 0)
    want = np.zeros(nk, np.uint16)
    alts = []
    if nk == 0:
        return want, alts
    f_lo, f_hi = _window_words(codes, k)
    r_lo, r_hi = _window_words((codes ^ 2)[::-1].copy(), k)
    r_lo, r_hi = r_lo[::-1], r_hi[::-1]  # r_*[p] = reverse complement of the k-mer at p
    _, skm_n, lo, hi, idx, _ = O.enumerate(read, k, m)
    p = t = 0
    for n in skm_n:
        n = int(n)
        vlo, vhi, vidx = lo[t:t + n], hi[t:t + n], idx[t:t + n]
        fwd = np.array_equal(vlo, f_lo[p:p + n]) and np.array_equal(vhi, f_hi[p:p + n])
        rev = np.array_equal(vlo, r_lo[p:p + n][::-1]) and np.array_equal(vhi, r_hi[p:p + n][::-1])
        assert fwd or rev, ("a vector that is neither the read's k-mers nor their reverse complements", read[:80], p, n)
        vals = np.array([0 if c < 0 else 0x100 | c for c in (O.index_get(h, int(a), int(b), int(i)) for a, b, i in zip(vlo, vhi, vidx))], np.uint16)
        want[p:p + n] = vals if fwd else vals[::-1]
        if fwd and rev:
            alts.append((p, p + n, vals[::-1].copy()))
        p += n
        t += n
    assert p == nk, (p, nk)
    return want, alts


def expected_all(O, h, reads, k, m):
    base = [0]
    parts, alts = [], []
    for r in reads:
        w, a = expected_slots(O, h, r, k, m)
        alts += [(base[-1] + s, base[-1] + e, v) for s, e, v in a]
        parts.append(w)
        base.append(base[-1] + len(w))
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint16)), alts, np.array(base, np.uint64)


def assert_slots(got, want, alts, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    if len(bad):
        ok = np.zeros(len(got), bool)
        for s, e, v in alts:
            if np.array_equal(got[s:e], v):
                ok[s:e] = True
        assert ok[bad].all(), (what, int(bad[~ok[bad]][0]), int(got[bad[~ok[bad]][0]]), int(want[bad[~ok[bad]][0]]), int((~ok[bad]).sum()))


def oracle_index(O, reads, k, m, b):
    h = O.index_new(k, m, b)
    flat, offs = oracle.pack_reads(reads)
    O.index_insert_reads(h, flat, offs)
    return h


def as_u16(counts, found):
    return np.where(found, 0x100 | counts.astype(np.uint16), 0).astype(np.uint16)


def packed_on_device(ix, seqs):
    import torch
    flat, offs = oracle.pack_reads(seqs)
    if len(flat) == 0:
        flat = np.zeros(1, np.uint8)
    d_bases = torch.from_numpy(flat).cuda()
    d_packed = torch.zeros((len(flat) + 15) // 16 + 4, dtype=torch.int32, device="cuda")
    d_starts = torch.from_numpy(offs.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    ix.pack_ascii(d_bases.data_ptr(), len(flat), d_packed.data_ptr())
    ix.sync()
    return d_packed, d_starts, offs


def get_kmers_packed(B, ix, seqs):
    import torch
    d_packed, d_starts, offs = packed_on_device(ix, seqs)
    total = int(B.kmer_slots(offs, ix.k)[-1])
    d_out = torch.full((max(total, 1),), 0x7777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ix.get_kmers_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), d_out.data_ptr())
    return d_out.cpu().numpy().view(np.uint16)[:total]


def query_set(rng, reads, k):
    absent = _random_reads(rng, 60, 4000)  # a genome the index never saw: (nearly) every slot absent
    partly = [r[:75] + "".join(rng.choice("ACGT") for _ in range(75)) for r in reads[:40]]  # half known, half not
    short = ["", "A", reads[0][:k - 1], reads[1][:k], reads[2][:k + 1], "ACGT" * 5]
    periodic = ["AC" * 100, "ACGTTGCA" * 30, "A" * 70 + "ACGTTGCA" * 10, "T" * 149 + "A", "ACGTTGCATGCA" * 13]
    return reads[:300] + SPECIAL + periodic + absent + partly + short


@pytest.mark.parametrize("k,m,b", GEOMETRIES)
def test_every_slot_matches_the_oracle(B, O, k, m, b):
    rng = random.Random(k * 100 + m + b)
    reads = _random_reads(rng, 1500, 3000) + SPECIAL + ["A" * 150] * 5 + ["ACGT" * 40] * 3
    queries = query_set(rng, reads, k)
    h = oracle_index(O, reads, k, m, b)
    want, alts, base = expected_all(O, h, queries, k, m)
    O.index_free(h)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(reads)
        counts, found, got_base = ix.get_kmers(queries)
        assert np.array_equal(got_base, base)
        got = as_u16(counts, found)
        assert_slots(got, want, alts, (k, m, b, "get_kmers"))
        assert found.sum() > len(found) // 3 and (~found).sum() > 0  # present and absent slots both exercised
        assert np.array_equal(get_kmers_packed(B, ix, queries), got), (k, m, b, "get_kmers_packed")


def test_inserted_reads_are_all_found_and_cover_get_reads(B, O):
    """Every slot of an inserted read is found, and a read's counts over its slots add up to at least its get_reads sum (that stop
    can only drop k-mers)."""
    rng = random.Random(3)
    reads = _random_reads(rng, 2000, 5000) + SPECIAL
    with B.BriskHip(63, 21, 14) as ix:
        ix.insert_reads(reads)
        counts, found, base = ix.get_kmers(reads)
        sums = ix.get_reads(reads)
    assert found.all()
    per_read = np.add.reduceat(counts.astype(np.uint64), base[:-1].astype(np.int64)) if len(counts) else np.zeros(0)
    assert (per_read >= sums).all()


def test_counts_wrap_but_presence_stays(B, O):
    """A k-mer inserted 256 times has count 0 mod 256 and reads back as 0x100: present."""
    rng = random.Random(256)
    for k, m, b in ((63, 21, 14), (31, 11, 11)):
        r256 = "".join(rng.choice("ACGT") for _ in range(k))
        r255 = "".join(rng.choice("ACGT") for _ in range(k + 3))
        reads = [r256] * 256 + [r255] * 255
        with B.BriskHip(k, m, b) as ix:
            ix.insert_reads(reads)
            counts, found, base = ix.get_kmers([r256, r255, "C" * k])
        assert list(base) == [0, 1, 5, 6]
        assert found[0] and counts[0] == 0
        assert found[1:5].all() and (counts[1:5] == 255).all()
        h = oracle_index(O, reads, k, m, b)
        want, alts, _ = expected_all(O, h, [r256, r255, "C" * k], k, m)
        O.index_free(h)
        assert_slots(as_u16(counts, found), want, alts, (k, m, b))


def test_long_sequences_are_answered_through_chunks(B, O):
    """Sequences of more than 8192 k-mers are scanned as chunks (re-scanned where a seam does not match: homopolymers, tandem
    repeats); a chunk's records are placed by their sequence's slot base."""
    rng = random.Random(2025)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    seqs = [rnd(60_017), rnd(8192 + 63), "A" * 30_000, "ACGTTGCA" * 4000, rnd(15_000) + "T" * 20_000 + rnd(15_000),
            rnd(5000) + "ACGTTGCA" * 3000 + rnd(5000) + rnd(64) * 200 + rnd(3000), rnd(2500) + "CA" * 9000 + rnd(2500)]
    seqs += _random_reads(rng, 200, 3000)
    queries = seqs + [rnd(20_000) + "A" * 90 + rnd(20_000), "A" * 70 + rnd(30_000)] + _random_reads(rng, 50, 3000)
    for k, m, b in ((63, 21, 14), (31, 11, 11), (31, 15, 14)):
        h = oracle_index(O, seqs, k, m, b)
        want, alts, base = expected_all(O, h, queries, k, m)
        O.index_free(h)
        with B.BriskHip(k, m, b) as ix:
            ix.insert_reads(seqs)
            counts, found, got_base = ix.get_kmers(queries)
            assert np.array_equal(got_base, base)
            got = as_u16(counts, found)
            assert_slots(got, want, alts, (k, m, b))
            assert np.array_equal(get_kmers_packed(B, ix, queries), got), (k, m, b, "packed")


def test_batching_does_not_change_the_answer(B, O):
    rng = random.Random(11)
    reads = _random_reads(rng, 3000, 6000) + SPECIAL
    queries = query_set(rng, reads, 63)
    outs = []
    for kw in ({}, {"max_batch_reads": 97}, {"max_batch_reads": 1}):
        with B.BriskHip(63, 21, 14, **kw) as ix:
            ix.insert_reads(reads)
            outs.append(as_u16(*ix.get_kmers(queries)[:2]))
            if kw.get("max_batch_reads") == 97:
                assert np.array_equal(get_kmers_packed(B, ix, queries), outs[-1])
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    h = oracle_index(O, reads, 63, 21, 14)
    want, alts, _ = expected_all(O, h, queries, 63, 21)
    O.index_free(h)
    assert_slots(outs[0], want, alts)


def test_deferred_inserts_are_visible(B, O):
    """Small insert batches are scanned and held back (brisk_hip_options.immediate_inserts = 0); the get completes them first."""
    rng = random.Random(7)
    reads = _random_reads(rng, 500, 2000)
    with B.BriskHip(63, 21, 14) as ix:
        ix.insert_reads(reads[:250])
        ix.insert_reads(reads[250:])
        counts, found, base = ix.get_kmers(reads)
        assert found.all()
        h = oracle_index(O, reads, 63, 21, 14)
        want, alts, _ = expected_all(O, h, reads, 63, 21)
        O.index_free(h)
        assert_slots(as_u16(counts, found), want, alts)


def test_capacity_and_refusals(B, O):
    import ctypes as C
    from brisk_amd import hipapi
    reads = _random_reads(random.Random(5), 20, 500)
    flat, offs = oracle.pack_reads(reads)
    total = int(B.kmer_slots(offs, 31)[-1])
    with B.BriskHip(31, 15, 14) as ix:
        ix.insert_reads(reads)
        out = np.full(total, 0xabcd, np.uint16)
        rc = ix.L.brisk_hip_get_kmers(ix.h, flat, offs, len(reads), out, total - 1)
        assert rc == hipapi.ECAPACITY
        assert (out == 0xabcd).all()  # nothing written
        rc = ix.L.brisk_hip_get_kmers(ix.h, flat, offs, len(reads), out, total)
        assert rc == 0 and (out != 0xabcd).all() and ((out & 0x100) != 0).all()
    with B.BriskHip(31, 15, 14, entry_ids=True) as ix:
        with pytest.raises(B.BriskHipError) as e:
            ix.get_kmers(reads)
        assert e.value.code == 1 and "entry-id" in str(e.value)
    with B.BriskHip(31, 15, 14, n_owners=2, owner_rank=0) as ix:
        with pytest.raises(B.BriskHipError) as e:
            ix.get_kmers(reads)
        assert e.value.code == 1 and "sharded" in str(e.value)
        import torch
        d_packed, d_starts, _ = packed_on_device(ix, reads)
        d_out = torch.zeros(total, dtype=torch.int16, device="cuda")
        with pytest.raises(B.BriskHipError) as e:
            ix.get_kmers_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), d_out.data_ptr())
        assert e.value.code == 1


def test_kernel_variants_match_the_oracle(B):
    """The probe bodies and record layouts small inputs do not reach by themselves: the generic body, the classic layout, tiny bins
    (nearly every record overflows into the scatter), the workgroup-per-partition probe for (nearly) every partition.  The library
    reads these settings once per process: one child process each (tests/kmer_query_worker.py)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kmer_query_worker.py")
    for extra in ({"BRISK_QUERY_GENERIC": "1"}, {"BRISK_BINS": "0"}, {"BRISK_BINS": "2", "BRISK_QUERY_ENT": "256"},
                  {"BRISK_HUGE_QUERY_AT": "0"}, {"BRISK_HUGE_QUERY_AT": "0", "BRISK_BINS": "2"}, {"BRISK_HUGE_QUERY_AT": "8", "BRISK_BINS": "0"},
                  {"BRISK_SCAN_CAP0": "8", "BRISK_BINS": "0"}):  # the per-position scan to staging, overflowing at 8 records and run again at the exact bound
        env = dict(os.environ, **extra)
        p = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and p.stdout.strip().endswith("ok 4"), (extra, p.stdout[-2000:], p.stderr[-4000:])
