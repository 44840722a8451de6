"""GPU: read extraction.  The gather (brisk_hip_extract_packed) against the numpy extractor of extract_reference.py, byte for byte;
the rule kernel against intervals_from_profile; the composed calls (brisk_hip_trim_packed / _trim_reads) against the host route
get_kmers -> profile_from_slots -> intervals_from_profile -> Python slicing; unpack_ascii against pack_ascii; brisk_count --extract."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle
from extract_reference import extract_reference, pack_reads
from extract_worker import E2E_GEOMETRIES, FILL, OutBuffers, device_reads, end_to_end, error_reads, host_route
from test_gpu_parity import _random_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "extract_worker.py")
EINVAL, ECAPACITY = 1, 5


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


def gather_case(rng):
    """(reads, intervals): every (start % 16, len % 16), lengths from 1, runs of kept reads shorter than a word, dropped reads at the
    front, at the end and in runs"""
    lens, ivs = [], []

    def add(n, start=0, length=0):
        assert n >= 1 and start + length <= n <= 200
        lens.append(n)
        ivs.append((start, length))

    for _ in range(5):                      # dropped reads at the front
        add(rng.randint(1, 200))
    for a in range(16):                     # all 256 alignments of start and length
        for b in range(16):
            start, length = a + 16 * rng.choice((0, 1, 2)), (b or 16) + 16 * rng.choice((0, 0, 1, 3))
            add(start + length + rng.randint(0, 25), start, length)
            if rng.random() < 0.2:
                add(rng.randint(1, 200))
    for a in range(16):                     # the same starts with the shortest lengths
        for length in (1, 2, 3):
            add(a + length + rng.randint(0, 40), a, length)
    for _ in range(30):                     # a run of dropped reads
        add(rng.randint(1, 200))
    for i in range(120):                    # whole reads of 1 .. 7 nucleotides, back to back: several to a word
        add(1 + i % 7, 0, 1 + i % 7)
    for i in range(60):                     # and short cuts out of longer ones
        n = rng.randint(1, 200)
        length = rng.randint(1, min(n, 5))
        add(n, rng.randint(0, n - length), length)
    while len(lens) < 2000:                 # anything
        n = rng.randint(1, 200)
        if rng.random() < 0.35:
            add(n)
        else:
            start = rng.randrange(n)
            add(n, start, rng.randint(1, n - start))
    for i in range(20):
        add(1 + i % 3, 0, 1 + i % 3)
    for _ in range(5):                      # dropped reads at the end
        add(rng.randint(1, 200))
    reads = ["".join(rng.choice("ACGT") for _ in range(n)) for n in lens]
    return reads, ivs


def check_gather(B, ix, reads, ivs, with_index=True, cap=None):
    intervals = np.array(ivs, np.uint32).reshape(-1, 2).copy().view(B.READ_INTERVAL_DTYPE).reshape(-1)
    d_packed, d_starts, words, starts = device_reads(reads)
    want, want_starts, want_index, want_n, want_nts = extract_reference(words, starts, intervals)
    d_iv = to_device(intervals)
    out = OutBuffers(len(reads), len(words) if cap is None else cap)
    n_out, n_nts = ix.extract_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), d_iv.data_ptr(), out.packed.data_ptr(), out.cap, out.starts.data_ptr(),
                                     out.index.data_ptr() if with_index else None)
    got, got_starts, got_index = out.host()
    assert (n_out, n_nts) == (want_n, want_nts)
    assert np.array_equal(got[:len(want)], want)        # the used words, the zero bits that end the last one, the two zero words after
    assert (got[len(want):] == FILL).all()              # and nothing else
    assert np.array_equal(got_starts[:n_out + 1], want_starts) and (got_starts[n_out + 1:] == np.uint64(2**64 - 1)).all()
    if with_index:
        assert np.array_equal(got_index[:n_out], want_index) and (got_index[n_out:] == np.uint64(2**64 - 1)).all()
    else:
        assert (got_index == np.uint64(2**64 - 1)).all()
    return n_out, n_nts


def test_gather_against_the_numpy_reference(B):
    rng = random.Random(1616)
    reads, ivs = gather_case(rng)
    assert {(s % 16, n % 16) for s, n in ivs if n} == {(a, b) for a in range(16) for b in range(16)}
    assert min(n for _, n in ivs if n) == 1 and ivs[0][1] == 0 and ivs[-1][1] == 0 and len(reads) > 2000
    with B.BriskHip(31, 15, 14) as ix:
        n_out, n_nts = check_gather(B, ix, reads, ivs)
        assert 0 < n_out < len(reads) and n_nts > 256 * 16  # more than one block of output words
        check_gather(B, ix, reads, ivs, with_index=False)
        check_gather(B, ix, reads, ivs, cap=(n_nts + 15) // 16 + 2)                      # exactly the room it needs
        assert check_gather(B, ix, reads, [(0, len(r)) for r in reads])[0] == len(reads)  # everything kept: the stream itself
        assert check_gather(B, ix, reads, [(0, 0)] * len(reads)) == (0, 0)                # nothing kept
        assert check_gather(B, ix, [], []) == (0, 0)                                      # no reads
        assert check_gather(B, ix, ["ACGTT"], [(1, 3)]) == (1, 3)
        one = ["".join(rng.choice("ACGT") for _ in range(n)) for n in (16, 32, 1, 15)]    # outputs that end on a word boundary
        assert check_gather(B, ix, one, [(0, 16), (16, 16), (0, 0), (0, 0)]) == (2, 32)
        assert check_gather(B, ix, one, [(0, 0), (0, 0), (0, 1), (0, 15)]) == (2, 16)


def test_refusals(B):
    import torch
    rng = random.Random(3)
    reads = ["".join(rng.choice("ACGT") for _ in range(rng.randint(20, 120))) for _ in range(300)]
    good = [(2, len(r) - 5) for r in reads]
    with B.BriskHip(31, 15, 14) as ix:
        d_packed, d_starts, words, _ = device_reads(reads)

        def call(ivs, cap):
            d_iv = to_device(np.array(ivs, np.uint32))
            out = OutBuffers(len(reads), len(words))
            with pytest.raises(B.BriskHipError) as e:
                ix.extract_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), d_iv.data_ptr(), out.packed.data_ptr(), cap, out.starts.data_ptr(), out.index.data_ptr())
            assert out.untouched(), "a refused call wrote to its output"
            return e.value

        # an interval past its read: one nucleotide too many, in two reads; the first one is named
        bad = list(good)
        bad[211] = (0, len(reads[211]) + 1)
        bad[37] = (len(reads[37]) - 2, 3)
        e = call(bad, len(words))
        assert e.code == EINVAL and "read 37 " in str(e), str(e)
        bad = list(good)
        bad[299] = (len(reads[299]) + 1, 0)  # a dropped read's start counts too
        e = call(bad, len(words))
        assert e.code == EINVAL and "read 299 " in str(e), str(e)
        # room: one word too few
        n_nts = sum(n for _, n in good)
        e = call(good, (n_nts + 15) // 16 + 1)
        assert e.code == ECAPACITY and str((n_nts + 15) // 16 + 2) in str(e), str(e)
        assert check_gather(B, ix, reads, good, cap=(n_nts + 15) // 16 + 2) == (len(reads), n_nts)
        # null pointers
        d_iv = to_device(np.array(good, np.uint32))
        out = OutBuffers(len(reads), len(words))
        n1, n2 = C.c_uint64(), C.c_uint64()
        args = [ix.h, d_packed.data_ptr(), d_starts.data_ptr(), len(reads), d_iv.data_ptr(), out.packed.data_ptr(), out.cap, out.starts.data_ptr(), out.index.data_ptr(),
                C.byref(n1), C.byref(n2)]
        for hole in (0, 1, 2, 4, 5, 7, 9, 10):
            a = list(args)
            a[hole] = None
            assert ix.L.brisk_hip_extract_packed(*a) == EINVAL, hole
        assert out.untouched()
        # bad rules
        ix.insert_reads(reads)
        d_prof = to_device(ix.read_profile(reads))
        d_out = torch.zeros(len(reads) * 2, dtype=torch.int32, device="cuda")
        short = B.select_rule("median")
        short.struct_size = 16
        for rule in (B.select_rule(3), B.select_rule("median", lo=3, hi=2), B.select_rule("present", lo=1001, hi=1000), short):
            with pytest.raises(B.BriskHipError) as e:
                ix.select_intervals(d_prof.data_ptr(), len(reads), rule, d_out.data_ptr())
            assert e.value.code == EINVAL
            with pytest.raises(B.BriskHipError) as e:
                ix.trim_reads(reads, 2, rule)
            assert e.value.code == EINVAL
            with pytest.raises(B.BriskHipError) as e:
                ix.trim_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), out.packed.data_ptr(), out.cap, out.starts.data_ptr(), None, 2, rule)
            assert e.value.code == EINVAL
        assert ix.L.brisk_hip_select_intervals(ix.h, d_prof.data_ptr(), len(reads), None, d_out.data_ptr()) == EINVAL
        assert ix.L.brisk_hip_select_intervals(ix.h, None, len(reads), C.byref(B.select_rule("median")), d_out.data_ptr()) == EINVAL
        assert out.untouched()
        # a read table that does not ascend
        bad_starts = np.array(device_reads(reads)[3])
        bad_starts[3], bad_starts[4] = bad_starts[4], bad_starts[3]
        d_bad = to_device(bad_starts)
        with pytest.raises(B.BriskHipError) as e:
            ix.extract_packed(d_packed.data_ptr(), d_bad.data_ptr(), len(reads), d_iv.data_ptr(), out.packed.data_ptr(), out.cap, out.starts.data_ptr(), out.index.data_ptr())
        assert e.value.code == EINVAL and "ascend" in str(e.value) and out.untouched()
        # the handle is as it was
        assert len(ix.trim_reads(reads, 1)) == len(reads)


def test_a_stream_of_more_than_2_to_the_32_nucleotides(B):
    """30 M reads of 150 bp are 4.5 G nucleotides, the smallest bench-shaped input whose positions pass 2^32: every third read is
    kept at [7, 107), and sampled output reads -- those next to the crossing among them -- are compared with the same stretch of the
    input, both through unpack_ascii"""
    import torch
    n, L = 30_000_000, 150
    n_words = (n * L + 15) // 16
    with B.BriskHip(63, 21, 14) as ix:
        d_packed = torch.zeros(n_words + 4, dtype=torch.int32, device="cuda")
        d_starts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ix.synth_reads(1 << 24, 0, n, L, d_packed.data_ptr(), d_starts.data_ptr())
        ix.sync()
        keep = (torch.arange(n, device="cuda") % 3) == 0
        d_iv = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        d_iv[:, 0] = torch.where(keep, 7, 0)
        d_iv[:, 1] = torch.where(keep, 100, 0)
        n_keep = n // 3
        cap = (n_keep * 100 + 15) // 16 + 2
        d_out = torch.zeros(cap, dtype=torch.int32, device="cuda")
        d_os = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_oi = torch.zeros(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        n_out, n_nts = ix.extract_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_iv.data_ptr(), d_out.data_ptr(), cap, d_os.data_ptr(), d_oi.data_ptr())
        assert (n_out, n_nts) == (n_keep, n_keep * 100)
        assert int(d_os[0]) == 0 and int(d_os[n_out]) == n_nts
        ramp = torch.arange(n_out + 1, device="cuda", dtype=torch.int64)
        assert bool((d_os[:n_out + 1] == ramp * 100).all()) and bool((d_oi[:n_out] == ramp[:n_out] * 3).all())
        assert int(d_out[cap - 1]) == 0 and int(d_out[cap - 2]) == 0
        cross = (1 << 32) // L // 3  # the kept read at or before input position 2^32
        assert 3 * cross * L <= 1 << 32 < 3 * (cross + 1) * L
        rng = random.Random(32)
        sample = sorted({0, 1, n_out - 2, n_out - 1} | set(range(cross - 20, cross + 21)) | {rng.randrange(n_out) for _ in range(950)})
        d_a = torch.zeros(len(sample) * 100, dtype=torch.uint8, device="cuda")
        d_b = torch.zeros(len(sample) * 100, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for i, j in enumerate(sample):
            ix.unpack_ascii(d_out.data_ptr(), j * 100, 100, d_a.data_ptr() + i * 100)
            ix.unpack_ascii(d_packed.data_ptr(), 3 * j * L + 7, 100, d_b.data_ptr() + i * 100)
        ix.sync()
        a, b = d_a.cpu().numpy().reshape(-1, 100), d_b.cpu().numpy().reshape(-1, 100)
        assert set(np.unique(b).tolist()) == {65, 67, 71, 84}
        bad = np.nonzero((a != b).any(axis=1))[0]
        assert len(bad) == 0, [sample[i] for i in bad[:10]]
        assert len({r.tobytes() for r in b}) > 900  # the sampled reads differ from one another: a shifted copy would not pass


def rules_for(mid):
    """mid: a median count that some reads lie above and some do not (it depends on k: the coverage in k-mers does)"""
    return [("solid_run", {}), ("solid_run", dict(min_len=100)), ("solid_run", dict(min_len=151)), ("median", dict(lo=0, hi=mid)), ("median", dict(lo=mid + 1, hi=255)),
            ("median", dict(lo=1, hi=255, min_len=120)), ("present", dict(lo=1000, hi=1000)), ("present", dict(lo=0, hi=899)), ("present", dict(lo=900, hi=999, min_len=101))]


@pytest.mark.parametrize("k,m,b", E2E_GEOMETRIES)
def test_rule_kernel_equals_intervals_from_profile(B, k, m, b):
    import torch
    seqs = error_reads(k)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(seqs[:2 * len(seqs) // 3])  # (the other reads' errors are k-mers the index does not hold)
        prof = ix.read_profile(seqs, 2)
        assert (prof["n_kmers"] == 0).any() and (prof["run_len"] < prof["n_kmers"]).any() and (prof["n_present"] < prof["n_kmers"]).any()
        d_prof = to_device(prof)
        for kind, kw in rules_for(int(np.median(prof["median"][prof["n_kmers"] > 0]))):
            rule = B.select_rule(kind, **kw)
            want = B.intervals_from_profile(prof, k, rule)
            d_iv = torch.full((len(seqs) * 2,), 0x77777777, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ix.select_intervals(d_prof.data_ptr(), len(seqs), rule, d_iv.data_ptr())
            got = d_iv.cpu().numpy().view(B.READ_INTERVAL_DTYPE)
            assert np.array_equal(got, want), (kind, kw, int(np.nonzero(got != want)[0][0]))
            assert 0 < (want["len"] > 0).sum() < len(seqs), (kind, kw, "the rule does not tell the reads apart")
            assert np.array_equal(ix.trim_reads(seqs, 2, rule), want), (kind, kw, "trim_reads")


@pytest.mark.parametrize("k,m,b", E2E_GEOMETRIES)
def test_trim_on_the_device_and_recount(B, k, m, b):
    end_to_end(k, m, b, max_batch_reads=97)


def test_trim_and_recount_with_segmented_profiles(B):
    """BRISK_PROFILE_SEG is read once per process: a child, in which every read of more than 64 slots is profiled in segments"""
    p = subprocess.run([sys.executable, WORKER], env=dict(os.environ, BRISK_PROFILE_SEG="64"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok 2"), (p.stdout[-2000:], p.stderr[-4000:])


def test_trim_reads_and_trim_packed_agree_and_complete_deferred_inserts(B):
    rng = random.Random(7)
    reads = _random_reads(rng, 500, 2000)
    whole = np.zeros(len(reads), B.READ_INTERVAL_DTYPE)
    whole["len"] = 150
    with B.BriskHip(63, 21, 14) as ix:  # two small insert calls: deferred until a call needs the index
        ix.insert_reads(reads[:250])
        ix.insert_reads(reads[250:])
        assert np.array_equal(ix.trim_reads(reads, 1), whole)
    with B.BriskHip(63, 21, 14) as ix:
        ix.insert_reads(reads[:250])
        ix.insert_reads(reads[250:])
        d_packed, d_starts, words, starts = device_reads(reads)
        out = OutBuffers(len(reads), len(words))
        assert ix.trim_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), out.packed.data_ptr(), out.cap, out.starts.data_ptr(), out.index.data_ptr(), 1) == (500, 75000)
        got, got_starts, got_index = out.host()
        assert np.array_equal(got[:len(words)], words) and np.array_equal(got_starts[:501], starts) and got_index[:500].tolist() == list(range(500))
    # reads with errors: what trim_packed writes is what the intervals of trim_reads cut out of the stream
    for k, m, b in E2E_GEOMETRIES:
        seqs = error_reads(k, 1500, seed=11)
        with B.BriskHip(k, m, b) as ix:
            ix.insert_reads(seqs[:1000])
            d_packed, d_starts, words, starts = device_reads(seqs)
            for rule in (B.select_rule("solid_run"), B.select_rule("median", lo=3, hi=255, min_len=90), B.select_rule("present", lo=0, hi=950)):
                ivs = ix.trim_reads(seqs, 2, rule)
                assert np.array_equal(ivs, host_route(ix, seqs, 2, rule)[0])
                want, want_starts, want_index, want_n, want_nts = extract_reference(words, starts, ivs)
                out = OutBuffers(len(seqs), len(words))
                got_n = ix.trim_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), out.packed.data_ptr(), out.cap, out.starts.data_ptr(), out.index.data_ptr(), 2, rule)
                got, got_starts, got_index = out.host()
                assert got_n == (want_n, want_nts) and 0 < want_n < len(seqs)
                assert np.array_equal(got[:len(want)], want) and (got[len(want):] == FILL).all()
                assert np.array_equal(got_starts[:want_n + 1], want_starts) and np.array_equal(got_index[:want_n], want_index)


def test_sharded_and_entry_id_handles(B):
    rng = random.Random(5)
    reads = _random_reads(rng, 20, 500)
    ivs = [(i % 7, 150 - 2 * (i % 7) - i) for i in range(len(reads))]
    for kw, word in ((dict(entry_ids=True), "entry-id"), (dict(n_owners=2, owner_rank=0), "sharded")):
        with B.BriskHip(31, 15, 14, **kw) as ix:
            with pytest.raises(B.BriskHipError) as e:
                ix.trim_reads(reads)
            assert e.value.code == EINVAL and word in str(e.value) and "trim_reads" in str(e.value)
            d_packed, d_starts, words, _ = device_reads(reads)
            out = OutBuffers(len(reads), len(words))
            with pytest.raises(B.BriskHipError) as e:
                ix.trim_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), out.packed.data_ptr(), out.cap, out.starts.data_ptr(), out.index.data_ptr())
            assert e.value.code == EINVAL and word in str(e.value) and "trim_packed" in str(e.value) and out.untouched()
            assert check_gather(B, ix, reads, ivs)[0] == len(reads)  # the gather needs no index


def test_unpack_ascii_inverts_pack_ascii(B):
    import torch
    rng = random.Random(8)
    x = "".join(rng.choice("ACGTacgt") for _ in range(333))
    with B.BriskHip(31, 15, 14) as ix:
        d_bases = torch.from_numpy(np.frombuffer(x.encode(), np.uint8).copy()).cuda()
        d_packed = torch.zeros((len(x) + 15) // 16, dtype=torch.int32, device="cuda")  # no word after the last used one: none may be read
        torch.cuda.synchronize()
        ix.pack_ascii(d_bases.data_ptr(), len(x), d_packed.data_ptr())
        ix.sync()
        for first in range(18):
            for n in (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100, 255, 256, 257, len(x) - first):
                for shift in (0, 1):  # an output that is 16-byte aligned, and one that is not
                    d_out = torch.full((n + 40,), 0x2e, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    ix.unpack_ascii(d_packed.data_ptr(), first, n, d_out.data_ptr() + shift)
                    ix.sync()
                    got = d_out.cpu().numpy().tobytes().decode()
                    assert got == "." * shift + x.upper()[first:first + n] + "." * (40 - shift), (first, n, shift)
        assert ix.L.brisk_hip_unpack_ascii(ix.h, None, 0, 5, d_out.data_ptr()) == EINVAL
        assert ix.L.brisk_hip_unpack_ascii(ix.h, None, 0, 0, None) == 0


def test_brisk_count_extract(B, tmp_path):
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe):
        B.build_apps()
    fasta = os.path.join(ROOT, "tests", "golden", "test.fa")
    seqs = oracle.fasta_sequences(open(fasta).read())
    k, m, b = 31, 11, 4
    path = str(tmp_path / "kept.fa")
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(seqs)
        kept_any = dropped_any = False
        for text, solid, extra, rule in (("trim", 1, [], B.select_rule("solid_run")), ("trim", 2, ["--min-len", "40"], B.select_rule("solid_run", min_len=40)),
                                         ("median:1:255", 2, [], B.select_rule("median", lo=1, hi=255)), ("present:0:999", 2, [], B.select_rule("present", lo=0, hi=999)),
                                         ("present:1000:1000", 2, ["--min-len", "100"], B.select_rule("present", lo=1000, hi=1000, min_len=100))):
            p = subprocess.run([exe, "--bulk", fasta, str(k), str(m), str(b), "--extract", path, "--rule", text, "--solid", str(solid)] + extra, capture_output=True, text=True,
                               timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
            ivs, kept = host_route(ix, seqs, solid, rule)
            want = "".join(">%d %d %d\n%s\n" % (i, ivs[i]["start"], ivs[i]["len"], s) for i, s in kept)
            assert open(path).read() == want, (text, extra)
            kept_any |= len(kept) > 0
            dropped_any |= len(kept) < len(seqs)
        assert kept_any and dropped_any
