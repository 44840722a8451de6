"""GPU: spectral read correction.  brisk_hip_weak_sites over crafted slots against sites_from_slots, row for row; the candidate
windows (brisk_hip_candidate_windows) against the numpy reference of correct_reference.py, byte for byte, and their refusals;
brisk_hip_decide_sites on crafted candidate slots; brisk_hip_apply_corrections against the numpy patch; the composed calls
(brisk_hip_correct_reads / _correct_packed) against the host route get_kmers -> sites_from_slots -> candidate strings -> get_kmers ->
corrections_from_candidates -> patched strings; planted substitutions restored; a crafted ambiguity; the recount of the corrected
stream; the independence of the batches; deferred inserts, sharded and entry-id handles; brisk_count --rule correct."""
import ctypes as C
import os
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle
from correct_reference import (LETTERS, as_corrections, as_sites, code_of, patch_reference, patch_strings, weak_cases, window_case, windows_reference)
from correct_worker import batches, check_against_route, route
from extract_reference import pack_reads
from extract_worker import E2E_GEOMETRIES, FILL, device_reads, error_reads
from split_reference import read_lengths
from split_worker import ROW_FILL, SplitBuffers, slot_words, to_device
from test_gpu_parity import _random_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "correct_worker.py")
EINVAL, ECAPACITY = 1, 5


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    assert brisk_amd.library_path()
    return brisk_amd


def child(args, **env):
    base = {k: v for k, v in os.environ.items() if k not in ("BRISK_PROFILE_BATCH", "BRISK_PROFILE_SEG", "BRISK_CORRECT_BATCH")}
    return subprocess.run([sys.executable, WORKER] + args, env=dict(base, **env), capture_output=True, text=True, timeout=600)


def site_rows(buf, n, B):
    return buf.host()[2][:n * 16].view(B.SITE_DTYPE)


def correction_rows(buf, n, B):
    return buf.host()[2][:n * 16].view(B.CORRECTION_DTYPE)


def test_weak_sites_on_crafted_slots(B):
    k = 9
    counts, found, base = weak_cases(random.Random(2727), k)
    lens = read_lengths(base, k)
    starts = np.zeros(len(base), np.uint64)
    starts[1:] = np.cumsum(lens, dtype=np.uint64)
    n_reads, seen = len(base) - 1, dict.fromkeys(("n_sites", "n_skip_whole", "n_skip_long", "n_skip_short"), 0)
    with B.BriskHip(k, 5, 2) as ix:
        d_slots, d_starts = to_device(slot_words(counts, found)), to_device(starts)
        for solid_min in (0, 1, 2, 255, 256):
            for min_cover in (1, k // 2, k, 0):
                want, want_st = B.sites_from_slots(counts, found, base, k, solid_min, min_cover)
                n = len(want)
                out = SplitBuffers(n)  # exactly the room it needs
                st = ix.weak_sites(d_slots.data_ptr(), d_starts.data_ptr(), n_reads, out.frags.data_ptr(), n, solid_min, min_cover)
                assert st == want_st, (solid_min, min_cover, st, want_st)
                got = site_rows(out, n, B)
                bad = np.nonzero(got != want)[0]
                assert len(bad) == 0, (solid_min, min_cover, int(bad[0]), got[bad[0]], want[bad[0]])
                p, s, f = out.host()
                assert (f[n * 16:] == ROW_FILL).all() and (p == FILL).all() and (s == np.uint64(2**64 - 1)).all()
                assert st["n_runs"] == st["n_sites"] + st["n_skip_whole"] + st["n_skip_long"] + st["n_skip_short"]
                for key in seen:
                    seen[key] += st[key]
                if n:  # one row too few: the stats filled, nothing written
                    out = SplitBuffers(n)
                    st = ix.weak_sites(d_slots.data_ptr(), d_starts.data_ptr(), n_reads, out.frags.data_ptr(), n - 1, solid_min, min_cover, raise_on_capacity=False)
                    assert st.pop("rc") == ECAPACITY and st == want_st and out.untouched(), (solid_min, min_cover)
        assert all(v > 0 for v in seen.values()), seen
        # refusals
        out = SplitBuffers(100)
        with pytest.raises(B.BriskHipError) as e:
            ix.weak_sites(d_slots.data_ptr(), d_starts.data_ptr(), n_reads, out.frags.data_ptr(), 100, 2, k + 1)
        assert e.value.code == EINVAL and "min_cover" in str(e.value)
        bad_starts = np.array(starts)
        bad_starts[3], bad_starts[4] = bad_starts[4] + 5, bad_starts[3]
        with pytest.raises(B.BriskHipError) as e:
            ix.weak_sites(d_slots.data_ptr(), to_device(bad_starts).data_ptr(), n_reads, out.frags.data_ptr(), 100, 2, 1)
        assert e.value.code == EINVAL and "ascend" in str(e.value)
        args = [ix.h, d_slots.data_ptr(), d_starts.data_ptr(), n_reads, 2, 0, out.frags.data_ptr(), 100, C.byref(B.hipapi._CorrectStats())]
        for hole in (0, 1, 2, 6, 8):
            a = list(args)
            a[hole] = None
            assert ix.L.brisk_hip_weak_sites(*a) == EINVAL, hole
        assert out.untouched()
        assert ix.weak_sites(0, 0, 0, 0, 0) == dict.fromkeys(B.CORRECT_STATS_FIELDS, 0)


def check_windows(B, ix, reads, rows, cap=None):
    k = ix.k
    sites = as_sites(rows)
    d_packed, d_starts, words, starts = device_reads(reads)
    want, want_starts, want_nts = windows_reference(words, starts, sites, k)
    d_sites = to_device(sites)
    out = SplitBuffers(3 * len(rows), len(want) if cap is None else cap)
    n_nts = ix.candidate_windows(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), d_sites.data_ptr(), len(rows), out.packed.data_ptr(), out.cap, out.starts.data_ptr())
    got, got_starts, got_rows = out.host()
    assert n_nts == want_nts
    bad = np.nonzero(got[:len(want)] != want)[0]
    assert len(bad) == 0, (int(bad[0]), hex(got[bad[0]]), hex(want[bad[0]]))
    assert (got[len(want):] == FILL).all()
    assert np.array_equal(got_starts[:3 * len(rows) + 1], want_starts) and (got_starts[3 * len(rows) + 1:] == np.uint64(2**64 - 1)).all()
    assert (got_rows == ROW_FILL).all()
    return n_nts


def test_candidate_windows_against_the_numpy_reference(B):
    k = 31
    reads, rows = window_case(random.Random(27), k)
    assert 3 * len(rows) > 256  # (test_correct_cpu.py checks what the case covers)
    with B.BriskHip(k, 15, 14) as ix:
        n_nts = check_windows(B, ix, reads, rows)
        assert n_nts > 2 * 256 * 16  # more than one block of output words
        check_windows(B, ix, reads, rows, cap=(n_nts + 15) // 16 + 2)
        assert check_windows(B, ix, reads, rows[::-1]) == n_nts  # any table, in its own order
        assert check_windows(B, ix, reads, []) == 0
        assert check_windows(B, ix, [], []) == 0
        one = "".join(random.Random(1).choice("ACGT") for _ in range(k))
        assert check_windows(B, ix, [one], [(0, 0, 1)]) == 3 * k
        assert check_windows(B, ix, [one], [(0, k - 1, 1)]) == 3 * k
        # refusals: each kind of bad row, the first one named; nothing written
        d_packed, d_starts, words, starts = device_reads(reads)
        good = list(rows)

        def call(table, cap, d_st=d_starts):
            d_sites = to_device(as_sites(table))
            out = SplitBuffers(3 * len(table), 4 * len(words) + 400)
            with pytest.raises(B.BriskHipError) as e:
                ix.candidate_windows(d_packed.data_ptr(), d_st.data_ptr(), len(reads), d_sites.data_ptr(), len(table), out.packed.data_ptr(), cap, out.starts.data_ptr())
            assert out.untouched(), "a refused call wrote to its output"
            return e.value

        r7, p7, c7 = good[7]
        for first in ((len(reads), 0, 1), (2**40, 0, 1), (r7, p7, 0), (r7, p7, k + 1), (r7, len(reads[r7]), 1), (r7, len(reads[r7]) - 1, k)):
            bad = list(good)
            bad[37], bad[111] = first, (len(reads) + 5, 0, 0)
            e = call(bad, 4 * len(words) + 400)
            assert e.code == EINVAL and "row 37 " in str(e), (first, str(e))
        e = call(good, (n_nts + 15) // 16 + 1)
        assert e.code == ECAPACITY and str((n_nts + 15) // 16 + 2) in str(e), str(e)
        bad_starts = np.array(starts)
        bad_starts[3], bad_starts[4] = bad_starts[4], bad_starts[3]
        e = call(good, 4 * len(words) + 400, to_device(bad_starts))
        assert e.code == EINVAL and "ascend" in str(e)
        d_sites = to_device(as_sites(good))
        out = SplitBuffers(3 * len(good), 4 * len(words) + 400)
        n_out = C.c_uint64()
        args = [ix.h, d_packed.data_ptr(), d_starts.data_ptr(), len(reads), d_sites.data_ptr(), len(good), out.packed.data_ptr(), out.cap, out.starts.data_ptr(), C.byref(n_out)]
        for hole in (0, 1, 2, 4, 6, 8, 9):
            a = list(args)
            a[hole] = None
            assert ix.L.brisk_hip_candidate_windows(*a) == EINVAL, hole
        assert out.untouched()
        assert check_windows(B, ix, reads, rows) == n_nts  # the handle is as it was


def test_decide_sites_on_crafted_candidate_slots(B):
    k = 31
    rng = random.Random(6)
    reads = ["".join(rng.choice("ACGT") for _ in range(3 * k + 40)) for _ in range(300)]
    rows, cc, cf = [], [], []
    for r in range(300):
        for pos, cover in ((k - 1, rng.randint(1, k)), (2 * k + 5, k)) if r % 3 else ((rng.randint(k - 1, 2 * k), k),):
            rows.append((r, pos, cover))
            passing = rng.sample(range(3), len(rows) % 4 if len(rows) < 40 else rng.choice((0, 1, 1, 1, 2, 3)))
            for c in range(3):
                cnt, fnd = [rng.choice((2, 3, 255)) for _ in range(cover)], [True] * cover
                if c not in passing:
                    x = rng.choice((0, cover - 1, rng.randrange(cover)))
                    fnd[x], cnt[x] = rng.random() < 0.5, 1
                cc += cnt
                cf += fnd
    sites = as_sites(rows)
    cc, cf = np.array(cc, np.uint8), np.array(cf, bool)
    frm = [code_of(reads[r][pos]) for r, pos, _ in rows]
    assert len(rows) > 256
    with B.BriskHip(k, 15, 14) as ix:
        d_packed, d_starts, words, starts = device_reads(reads)
        d_slots, d_sites = to_device(slot_words(cc, cf)), to_device(sites)
        for solid_min in (1, 2, 3, 256):
            want, cnt = B.corrections_from_candidates(cc, cf, sites, solid_min, frm)
            n = len(want)
            out = SplitBuffers(n)
            st = ix.decide_sites(d_slots.data_ptr(), d_sites.data_ptr(), len(rows), d_packed.data_ptr(), d_starts.data_ptr(), len(reads), out.frags.data_ptr(), n, solid_min)
            assert {key: st[key] for key in cnt} == cnt and sum(st.values()) == 2 * len(rows), (solid_min, st, cnt)
            assert np.array_equal(correction_rows(out, n, B), want) and (out.host()[2][n * 16:] == ROW_FILL).all()
            if solid_min == 2:
                assert cnt["n_corrected"] > 0 and cnt["n_ambiguous"] > 0 and cnt["n_unresolved"] > 0
            if n:
                out = SplitBuffers(n)
                st2 = ix.decide_sites(d_slots.data_ptr(), d_sites.data_ptr(), len(rows), d_packed.data_ptr(), d_starts.data_ptr(), len(reads), out.frags.data_ptr(), n - 1, solid_min,
                                      raise_on_capacity=False)
                assert st2.pop("rc") == ECAPACITY and st2 == st and out.untouched()
        bad = list(rows)
        bad[50] = (300, 5, 3)
        out = SplitBuffers(len(rows))
        with pytest.raises(B.BriskHipError) as e:
            ix.decide_sites(d_slots.data_ptr(), to_device(as_sites(bad)).data_ptr(), len(rows), d_packed.data_ptr(), d_starts.data_ptr(), len(reads), out.frags.data_ptr(), len(rows), 2)
        assert e.value.code == EINVAL and "row 50 " in str(e.value) and out.untouched()
        assert ix.decide_sites(0, 0, 0, d_packed.data_ptr(), d_starts.data_ptr(), len(reads), 0, 0) == dict.fromkeys(B.CORRECT_STATS_FIELDS, 0)


def test_apply_corrections_against_the_numpy_patch(B):
    rng = random.Random(9)
    reads = ["".join(rng.choice("ACGT") for _ in range(n)) for n in [16, 20, 12, 1, 0, 33] + [rng.randint(1, 200) for _ in range(600)]]
    words, starts = pack_reads(reads)

    def row(r, pos, to=None):
        f = code_of(reads[r][pos])
        return (r, pos, f, rng.choice([x for x in range(4) if x != f]) if to is None else to, 1)

    rows = [row(0, 0), row(0, 3), row(0, 15), row(1, 0), row(1, 19), row(2, 0)]  # the first word, twice; the word reads 1 and 2 share, from both
    for r in range(6, len(reads) - 1):
        if rng.random() < 0.5:
            rows += [row(r, pos) for pos in sorted(rng.sample(range(len(reads[r])), min(len(reads[r]), rng.choice((1, 2, 3)))))]
    last = len(reads) - 1
    rows.append(row(last, len(reads[last]) - 1))  # the last nucleotide of the stream
    table = as_corrections(rows)
    assert len(rows) > 256 and len(words) > 2 * 256
    with B.BriskHip(31, 15, 14) as ix:
        d_packed, d_starts = to_device(words), to_device(starts)

        def apply(t, cap=len(words), d_st=d_starts, n_reads=len(reads)):
            out = SplitBuffers(0, cap)
            ix.apply_corrections(d_packed.data_ptr(), d_st.data_ptr(), n_reads, to_device(t).data_ptr(), len(t), out.packed.data_ptr(), cap)
            p = out.host()[0]
            assert (p[len(words):] == FILL).all()
            return p[:len(words)]

        got = apply(table)
        assert np.array_equal(got, patch_reference(words, starts, table)) and np.array_equal(got, pack_reads(patch_strings(reads, table)[0])[0])
        assert np.array_equal(apply(as_corrections([])), words)
        assert np.array_equal(apply(table[:1]), patch_reference(words, starts, table[:1]))

        def refused(t, cap=len(words), d_st=d_starts):
            out = SplitBuffers(0, len(words))
            with pytest.raises(B.BriskHipError) as e:
                ix.apply_corrections(d_packed.data_ptr(), d_st.data_ptr(), len(reads), to_device(t).data_ptr(), len(t), out.packed.data_ptr(), cap)
            assert out.untouched(), "a refused call wrote to its output"
            return e.value

        r9, p9 = rows[99][0], rows[99][1]
        f9 = code_of(reads[r9][p9])
        for bad in ((len(reads), 0, 0, 1, 1), (r9, len(reads[r9]), f9, (f9 + 1) % 4, 1), (r9, p9, (f9 + 1) % 4, f9, 1), (r9, p9, f9, f9, 1), (r9, p9, f9, 7, 1), rows[98], rows[97]):
            t = as_corrections(rows)
            t[99] = bad
            e = refused(t)
            assert e.code == EINVAL and "row 99 " in str(e), (bad, str(e))
        e = refused(table, len(words) - 1)
        assert e.code == ECAPACITY and str(len(words)) in str(e)
        bad_starts = np.array(starts)
        bad_starts[8], bad_starts[9] = bad_starts[9], bad_starts[8]
        e = refused(table, d_st=to_device(bad_starts))
        assert e.code == EINVAL and "ascend" in str(e)
        assert np.array_equal(apply(table), got)


@pytest.mark.parametrize("k,m,b", E2E_GEOMETRIES)
def test_correct_reads_and_correct_packed_against_the_host_route(B, k, m, b):
    seqs = error_reads(k)
    n = len(seqs)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(seqs[:2 * n // 3])  # (the other reads' errors are k-mers the index does not hold)
        for solid_min, min_cover in ((2, 0), (2, 1), (1, k // 2), (256, 0)):
            p, rows, st, host_rows, host_st = check_against_route(ix, seqs, solid_min, min_cover)
            print(k, solid_min, min_cover, st)
            if solid_min == 256:  # no slot is solid: every read with a slot is one whole run
                assert st["n_runs"] == st["n_skip_whole"] == sum(len(s) >= k for s in seqs) and st["n_sites"] == 0 and st["n_weak"] == st["n_slots"] > 0
                assert np.array_equal(p, pack_reads(seqs)[0])
                continue
            assert st["n_corrected"] > 0 and st["n_unresolved"] > 0
            assert st["n_skip_whole"] > 0 and st["n_skip_long"] > 0 and st["n_skip_short"] > 0
            assert not np.array_equal(p, pack_reads(seqs)[0])


def planted_reads(k, seed=11):
    """(genome, error-free reads, the same reads with one substitution each, the positions)"""
    rng = random.Random(seed)
    genome = "".join(rng.choice("ACGT") for _ in range(6000))
    clean, bad, where, used = [], [], [], set()
    for i in range(400):
        n = rng.choice((2 * k + 10, 100, 150))
        pos = (0, 1, k - 2, k - 1, n // 2, n - k, n - 1)[i % 7]
        a = rng.randrange(len(genome) - n)
        while a + pos in used:  # no two reads change the same nucleotide of the genome: a mutated k-mer is seen once
            a = rng.randrange(len(genome) - n)
        used.add(a + pos)
        s = genome[a:a + n]
        clean.append(s)
        bad.append(s[:pos] + rng.choice([c for c in "ACGT" if c != s[pos]]) + s[pos + 1:])
        where.append(pos)
    return genome, clean, bad, where


@pytest.mark.parametrize("also_mutated", (False, True))
def test_planted_substitutions_are_restored(B, also_mutated):
    k, m, b = E2E_GEOMETRIES[1]
    _, clean, bad, where = planted_reads(k)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(clean + clean)  # every true k-mer has count at least 2
        if also_mutated:
            ix.insert_reads(bad)        # and the mutated ones count 1: still weak
        rows, st = ix.correct_reads(bad, 2, 1)
        patched, per_read = patch_strings(bad, rows)
        assert patched == clean and per_read == [1] * len(bad) and st["n_corrected"] == st["n_sites"] == st["n_runs"] == len(bad)
        assert rows["pos"].tolist() == where
        rows, st = ix.correct_reads(bad, 2, k)
        patched, per_read = patch_strings(bad, rows)
        inner = [k - 1 <= pos <= len(s) - k for s, pos in zip(bad, where)]
        assert per_read == [int(x) for x in inner] and 0 < sum(inner) < len(bad)
        assert all(p == (c if x else s) for p, c, s, x in zip(patched, clean, bad, inner))
        assert st["n_corrected"] == st["n_sites"] == sum(inner) and st["n_skip_short"] == len(bad) - sum(inner)
        rows, st = ix.correct_reads(clean, 2, 1)
        assert len(rows) == 0 and st["n_weak"] == 0 and st["n_slots"] > 0


def test_a_crafted_ambiguity_is_left_alone(B):
    k, m, b = E2E_GEOMETRIES[1]
    rng = random.Random(13)
    g1 = "".join(rng.choice("ACGT") for _ in range(400))
    g1 = g1[:200] + "A" + g1[201:]
    g2 = g1[:200] + "C" + g1[201:]
    read = g1[140:200] + "T" + g1[201:270]
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads([g1, g2, g1, g2])
        rows, st = ix.correct_reads([read, g1[140:270], g2[140:270]], 2, 1)
        assert len(rows) == 0 and (st["n_sites"], st["n_ambiguous"], st["n_corrected"], st["n_unresolved"], st["n_runs"], st["n_weak"]) == (1, 1, 0, 0, 1, k)
        d_packed, d_starts, words, _ = device_reads([read])
        out = SplitBuffers(1, len(words))
        st = ix.correct_packed(d_packed.data_ptr(), d_starts.data_ptr(), 1, out.packed.data_ptr(), len(words), out.frags.data_ptr(), 1, 2, 1)
        assert st["n_ambiguous"] == 1 and np.array_equal(out.host()[0][:len(words)], words) and (out.host()[2] == ROW_FILL).all()
        ix.insert_reads([g1])  # the third copy does not change the verdict: both candidates are solid
        assert ix.correct_reads([read], 2, 1)[1]["n_ambiguous"] == 1
        rows, st = ix.correct_reads([read], 3, 1)  # at solid_min 3 only g1's base passes
        assert [tuple(int(x) for x in t) for t in rows.tolist()] == [(0, 60, code_of("T"), code_of("A"), k)] and st["n_corrected"] == 1


@pytest.mark.parametrize("k,m,b", E2E_GEOMETRIES)
def test_recount_of_the_corrected_stream(B, k, m, b):
    """index A from error-bearing reads; B counts the stream correct_packed writes, C the host route's strings: the same index"""
    seqs = error_reads(k, 1500)
    with B.BriskHip(k, m, b) as A, B.BriskHip(k, m, b) as ixb, B.BriskHip(k, m, b) as ixc:
        A.insert_reads(seqs)
        d_packed, d_starts, words, _ = device_reads(seqs)
        out = SplitBuffers(0, len(words))
        st = A.correct_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), out.packed.data_ptr(), len(words), 0, 0, 2, 1)
        assert st["n_corrected"] > 0 and (out.host()[2] == ROW_FILL).all()  # no table was asked for
        ixb.insert_packed(out.packed.data_ptr(), d_starts.data_ptr(), len(seqs))  # the read table is the input's
        _, want_st, patched, _ = route(A, seqs, 2, 1)
        assert want_st == st
        ixc.insert_reads(patched)
        got, want = ixb.checksum(), ixc.checksum()
        before = A.checksum()
    assert got == want and got[0] > 0 and got != before, (k, got, want)


ENVIRONMENTS = {"whole": {}, "batch1": dict(BRISK_PROFILE_BATCH="1"), "batch5": dict(BRISK_PROFILE_BATCH="5"), "round1": dict(BRISK_CORRECT_BATCH="1"),
                "round7": dict(BRISK_CORRECT_BATCH="7")}
_outputs = {}


def outputs_of(name, tmp_path_factory):
    """the worker's bytes and stats in that environment (the library reads the two variables once per process): run once, shared by the tests"""
    if name not in _outputs:
        path = str(tmp_path_factory.mktemp("correct") / (name + ".pkl"))
        p = child(["batches", path], **ENVIRONMENTS[name])
        assert p.returncode == 0 and p.stdout.strip().endswith("ok 4"), (name, p.stdout[-2000:], p.stderr[-4000:])
        with open(path, "rb") as f:
            _outputs[name] = pickle.load(f)
    return _outputs[name]


def same_outputs(got, whole):
    assert len(whole) == 4 and sorted(got) == sorted(whole)
    assert [key for key in whole if got[key] != whole[key]] == []


def test_the_whole_call_in_one_batch(B, tmp_path_factory):
    assert len(outputs_of("whole", tmp_path_factory)) == 4  # (the worker has compared it with the host route)


@pytest.mark.parametrize("name", ("batch1", "batch5", "round1", "round7"))
def test_the_answer_does_not_depend_on_the_batches(B, name, tmp_path_factory):
    same_outputs(outputs_of(name, tmp_path_factory), outputs_of("whole", tmp_path_factory))


def test_the_answer_does_not_depend_on_max_batch_reads(B, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("correct") / "max97.pkl")
    assert batches(path, 97) == 4
    with open(path, "rb") as f:
        same_outputs(pickle.load(f), outputs_of("whole", tmp_path_factory))


def test_deferred_inserts_and_refused_handles(B):
    rng = random.Random(7)
    reads = _random_reads(rng, 500, 2000)
    bad = [s[:75] + LETTERS[(code_of(s[75]) + 1) % 4] + s[76:] for s in reads]
    k, m, b = E2E_GEOMETRIES[1]
    with B.BriskHip(k, m, b) as ix:  # two small insert calls: deferred until a call needs the index
        ix.insert_reads(reads[:250])
        ix.insert_reads(reads[250:])
        rows, st = ix.correct_reads(bad, 1)
        assert patch_strings(bad, rows)[0] == [s.upper() for s in reads] and st["n_corrected"] == 500
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(reads[:250])
        ix.insert_reads(reads[250:])
        d_packed, d_starts, words, starts = device_reads(bad)
        out = SplitBuffers(500, len(words))
        st = ix.correct_packed(d_packed.data_ptr(), d_starts.data_ptr(), 500, out.packed.data_ptr(), out.cap, out.frags.data_ptr(), 500, 1)
        assert st["n_corrected"] == 500 and np.array_equal(out.host()[0][:len(words)], pack_reads(reads)[0])
        stats = B.hipapi._CorrectStats()
        assert ix.L.brisk_hip_correct_packed(ix.h, d_packed.data_ptr(), d_starts.data_ptr(), 500, 1, 0, None, 5, None, 0, C.byref(stats)) == EINVAL
        assert ix.L.brisk_hip_correct_packed(ix.h, d_packed.data_ptr(), d_starts.data_ptr(), 500, 1, 0, None, 0, None, 5, C.byref(stats)) == EINVAL
        assert ix.L.brisk_hip_correct_packed(ix.h, d_packed.data_ptr(), d_starts.data_ptr(), 500, 1, 64, None, 0, None, 0, C.byref(stats)) == EINVAL
    small = _random_reads(rng, 20, 500)
    for kw, word in ((dict(entry_ids=True), "entry-id"), (dict(n_owners=2, owner_rank=0), "sharded")):
        with B.BriskHip(31, 15, 14, **kw) as ix:
            with pytest.raises(B.BriskHipError) as e:
                ix.correct_reads(small)
            assert e.value.code == EINVAL and word in str(e.value) and "correct_reads" in str(e.value)
            d_packed, d_starts, words, starts = device_reads(small)
            out = SplitBuffers(20, len(words))
            with pytest.raises(B.BriskHipError) as e:
                ix.correct_packed(d_packed.data_ptr(), d_starts.data_ptr(), 20, out.packed.data_ptr(), out.cap, out.frags.data_ptr(), 20)
            assert e.value.code == EINVAL and word in str(e.value) and "correct_packed" in str(e.value) and out.untouched()
            # the four building blocks need no index
            slots = np.full(20 * 120, 0x103, np.uint16)
            for r in range(20):
                slots[r * 120 + 40:r * 120 + 71] = 0x101
            sites = SplitBuffers(20)
            st = ix.weak_sites(to_device(slots).data_ptr(), d_starts.data_ptr(), 20, sites.frags.data_ptr(), 20, 2)
            table = site_rows(sites, 20, B).copy()
            assert st["n_sites"] == 20 and table.tolist() == [(r, 70, 31) for r in range(20)]
            assert check_windows(B, ix, small, table.tolist()) == 20 * 3 * 61
            cand = np.full(20 * 3 * 31, 0x103, np.uint16)
            for r in range(20):
                cand[r * 93:r * 93 + 31] = 0x101          # candidate 0 fails
                if r % 2:
                    cand[r * 93 + 40] = 0                 # and, for odd reads, candidate 1: one passes
            rows = SplitBuffers(20)
            st = ix.decide_sites(to_device(cand).data_ptr(), sites.frags.data_ptr(), 20, d_packed.data_ptr(), d_starts.data_ptr(), 20, rows.frags.data_ptr(), 20, 2)
            assert (st["n_corrected"], st["n_ambiguous"], st["n_unresolved"]) == (10, 10, 0)
            corr = correction_rows(rows, 10, B).copy()
            assert corr["read"].tolist() == list(range(1, 20, 2)) and all(int(t["to"]) == [x for x in range(4) if x != code_of(small[int(t["read"])][70])][2] for t in corr)
            fixed = SplitBuffers(0, len(words))
            ix.apply_corrections(d_packed.data_ptr(), d_starts.data_ptr(), 20, rows.frags.data_ptr(), 10, fixed.packed.data_ptr(), len(words))
            assert np.array_equal(fixed.host()[0][:len(words)], patch_reference(words, starts, corr))


def test_brisk_count_rule_correct(B, tmp_path):
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe):
        B.build_apps()
    fasta = os.path.join(ROOT, "tests", "golden", "test.fa")
    seqs = oracle.fasta_sequences(open(fasta).read())
    k, m, b = 31, 11, 4
    path = str(tmp_path / "corrected.fa")
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(seqs)
        for solid, extra, cover in ((2, [], 0), (2, ["--min-cover", "1"], 1), (1, ["--min-cover", "15"], 15)):
            p = subprocess.run([exe, "--bulk", fasta, str(k), str(m), str(b), "--extract", path, "--rule", "correct", "--solid", str(solid)] + extra, capture_output=True, text=True,
                               timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
            rows, st, patched, per_read = route(ix, seqs, solid, cover)
            want = "".join(">%d %d\n%s\n" % (r, n, s if n else seqs[r]) for r, (s, n) in enumerate(zip(patched, per_read)))
            assert open(path).read() == want, (solid, extra)
            assert "%d corrections in %d of %d reads, %d sites (%d ambiguous, %d unresolved) of %d weak runs (%d whole, %d long, %d short), %d of %d k-mers weak" % (
                st["n_corrected"], sum(n > 0 for n in per_read), st["n_reads"], st["n_sites"], st["n_ambiguous"], st["n_unresolved"], st["n_runs"], st["n_skip_whole"], st["n_skip_long"],
                st["n_skip_short"], st["n_weak"], st["n_slots"]) in p.stderr
    p = subprocess.run([exe, "--bulk", fasta, str(k), str(m), str(b), "--extract", path, "--rule", "corrects"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 2 and "--rule: trim, median:LO:HI or present:LO:HI, got corrects" in p.stderr  # a wrong rule exits as before
    p = subprocess.run([exe, "--bulk", fasta, str(k), str(m), str(b), "--extract", path, "--rule", "correct", "--paired"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 2 and "--paired" in p.stderr
    p = subprocess.run([exe, "--bulk", fasta, str(k), str(m), str(b), "--extract", path, "--rule", "split", "--min-cover", "3"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 2 and "--min-cover" in p.stderr
