"""GPU: read splitting.  brisk_hip_solid_runs over crafted slots against fragments_from_slots, row for row; the fragment gather
(brisk_hip_extract_fragments_packed) against the numpy gather of split_reference.py, byte for byte, and its refusals; the composed
calls (brisk_hip_split_reads / _split_packed) against the host route get_kmers -> fragments_from_slots -> gather_reference; the
recount of the fragments; the independence of the batches; deferred inserts, sharded and entry-id handles; brisk_count --rule split."""
import ctypes as C
import os
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle
from extract_worker import E2E_GEOMETRIES, FILL, device_reads, error_reads
from split_reference import as_table, fragment_case, gather_reference
from split_worker import ROW_FILL, SplitBuffers, batches, crafted_runs, split_outputs, to_device
from test_gpu_parity import _random_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "split_worker.py")
EINVAL, ECAPACITY = 1, 5


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    assert brisk_amd.library_path()
    return brisk_amd


def child(args, **env):
    base = {k: v for k, v in os.environ.items() if k not in ("BRISK_PROFILE_BATCH", "BRISK_PROFILE_SEG")}
    return subprocess.run([sys.executable, WORKER] + args, env=dict(base, **env), capture_output=True, text=True, timeout=600)


def test_solid_runs_on_crafted_slots(B):
    assert crafted_runs() == 20  # five solid_min, four min_len


def test_solid_runs_with_segmented_profiles(B):
    """BRISK_PROFILE_SEG is read once per process: a child (the run passes have no segments; the answer is the same)"""
    p = child(["runs"], BRISK_PROFILE_SEG="64")
    assert p.returncode == 0 and p.stdout.strip().endswith("ok 20"), (p.stdout[-2000:], p.stderr[-4000:])


def check_fragment_gather(B, ix, reads, rows, cap=None):
    table = as_table(rows)
    d_packed, d_starts, words, starts = device_reads(reads)
    want, want_starts, want_nts = gather_reference(words, starts, table)
    d_frags = to_device(table)
    out = SplitBuffers(len(rows), len(want) if cap is None else cap)
    n_nts = ix.extract_fragments_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), d_frags.data_ptr(), len(rows), out.packed.data_ptr(), out.cap, out.starts.data_ptr())
    got, got_starts, got_rows = out.host()
    assert n_nts == want_nts
    assert np.array_equal(got[:len(want)], want)        # the used words, the zero bits that end the last one, the two zero words after
    assert (got[len(want):] == FILL).all()              # and nothing else
    assert np.array_equal(got_starts[:len(rows) + 1], want_starts) and (got_starts[len(rows) + 1:] == np.uint64(2**64 - 1)).all()
    assert (got_rows == ROW_FILL).all()
    return n_nts


def test_fragment_gather_against_the_numpy_reference(B):
    rng = random.Random(2626)
    reads, rows = fragment_case(rng)
    assert {(s % 16, n % 16) for _, s, n in rows} == {(a, b) for a in range(16) for b in range(16)}
    per_read = np.bincount([r for r, _, _ in rows], minlength=len(reads))
    assert {1, 2, 3} <= {n for _, _, n in rows} and (per_read == 0).any() and (per_read >= 3).any()
    assert any(a == b for a, b in zip(rows, rows[1:])) and any(a[0] == b[0] and b[1] < a[1] + a[2] for a, b in zip(rows, rows[1:]))
    with B.BriskHip(31, 15, 14) as ix:
        n_nts = check_fragment_gather(B, ix, reads, rows)
        assert n_nts > 2 * 256 * 16 and len(rows) > 256                                    # more than one block of output words and of rows' lanes
        check_fragment_gather(B, ix, reads, rows, cap=(n_nts + 15) // 16 + 2)             # exactly the room it needs
        whole = [(r, 0, len(s)) for r, s in enumerate(reads)]
        n_in = sum(len(s) for s in reads)
        assert check_fragment_gather(B, ix, reads, whole) == n_in                          # every read once: the stream itself
        assert check_fragment_gather(B, ix, reads, [w for w in whole for _ in (0, 1)]) == 2 * n_in  # more nucleotides out than in
        assert check_fragment_gather(B, ix, reads, rows[::-1]) == n_nts                    # any order: the table's
        assert check_fragment_gather(B, ix, reads, []) == 0                                # the empty table
        assert check_fragment_gather(B, ix, [], []) == 0
        assert check_fragment_gather(B, ix, ["ACGTT"], [(0, 1, 3), (0, 0, 5)]) == 8
        one = ["".join(rng.choice("ACGT") for _ in range(n)) for n in (16, 32, 1, 15)]     # outputs that end on a word boundary
        assert check_fragment_gather(B, ix, one, [(0, 0, 16), (1, 16, 16)]) == 32
        assert check_fragment_gather(B, ix, one, [(2, 0, 1), (3, 0, 15)]) == 16


def test_fragment_gather_refusals(B):
    rng = random.Random(3)
    reads = ["".join(rng.choice("ACGT") for _ in range(rng.randint(20, 120))) for _ in range(300)]
    good = [(r, 2, len(s) - 5) for r, s in enumerate(reads)] + [(r, 0, 7) for r in range(0, 300, 3)]
    with B.BriskHip(31, 15, 14) as ix:
        d_packed, d_starts, words, starts = device_reads(reads)

        def call(rows, cap, d_st=d_starts):
            d_frags = to_device(as_table(rows))
            out = SplitBuffers(len(rows), 2 * len(words))
            with pytest.raises(B.BriskHipError) as e:
                ix.extract_fragments_packed(d_packed.data_ptr(), d_st.data_ptr(), len(reads), d_frags.data_ptr(), len(rows), out.packed.data_ptr(), cap, out.starts.data_ptr())
            assert out.untouched(), "a refused call wrote to its output"
            return e.value

        # each kind of bad row, two of them: the first one is named
        for first, second in (((300, 0, 5), (2**40, 0, 5)), ((7, 3, 0), (8, 0, 0)), ((7, 0, len(reads[7]) + 1), (9, len(reads[9]) - 2, 3)), ((7, len(reads[7]), 1), (300, 0, 0))):
            bad = list(good)
            bad[37], bad[211] = first, second
            e = call(bad, 2 * len(words))
            assert e.code == EINVAL and "row 37 " in str(e), str(e)
            bad = list(good)
            bad[len(bad) - 1] = first
            e = call(bad, 2 * len(words))
            assert e.code == EINVAL and "row %d " % (len(bad) - 1) in str(e), str(e)
        # room: one word too few
        n_nts = sum(n for _, _, n in good)
        e = call(good, (n_nts + 15) // 16 + 1)
        assert e.code == ECAPACITY and str((n_nts + 15) // 16 + 2) in str(e), str(e)
        n_out = C.c_uint64()
        d_frags = to_device(as_table(good))
        out = SplitBuffers(len(good), 2 * len(words))
        args = [ix.h, d_packed.data_ptr(), d_starts.data_ptr(), len(reads), d_frags.data_ptr(), len(good), out.packed.data_ptr(), (n_nts + 15) // 16 + 1, out.starts.data_ptr(), C.byref(n_out)]
        assert ix.L.brisk_hip_extract_fragments_packed(*args) == ECAPACITY and n_out.value == n_nts and out.untouched()  # the count is filled
        assert check_fragment_gather(B, ix, reads, good, cap=(n_nts + 15) // 16 + 2) == n_nts
        # null pointers
        args[7] = out.cap
        for hole in (0, 1, 2, 4, 6, 8, 9):
            a = list(args)
            a[hole] = None
            assert ix.L.brisk_hip_extract_fragments_packed(*a) == EINVAL, hole
        assert out.untouched()
        # a read table that does not ascend
        bad_starts = np.array(starts)
        bad_starts[3], bad_starts[4] = bad_starts[4], bad_starts[3]
        e = call(good, 2 * len(words), to_device(bad_starts))
        assert e.code == EINVAL and "ascend" in str(e)
        assert check_fragment_gather(B, ix, reads, good) == n_nts  # the handle is as it was


@pytest.mark.parametrize("k,m,b", E2E_GEOMETRIES)
def test_split_reads_and_split_packed_against_the_host_route(B, k, m, b):
    """n_short > 0 is asserted where it can hold: at min_len 0 every solid run covers k nucleotides and is a fragment"""
    seqs = error_reads(k)
    n = len(seqs)
    words, starts = device_reads(seqs)[2:]
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(seqs[:2 * n // 3])  # (the other reads' errors are k-mers the index does not hold)
        slots = ix.get_kmers(seqs)
        for solid_min, min_len in ((2, 0), (2, k + 20), (1, 0), (256, 0)):
            want, want_st = B.fragments_from_slots(*slots, k, solid_min, min_len, n_nts_in=int(starts[-1]))
            p, s, rows, st, host_rows, host_st = split_outputs(ix, seqs, solid_min, min_len)
            assert np.array_equal(host_rows, want) and host_st == want_st, (solid_min, min_len, "split_reads")
            assert np.array_equal(rows, want) and st == want_st, (solid_min, min_len, "split_packed")
            want_p, want_s, want_nts = gather_reference(words, starts, want)
            assert np.array_equal(p, want_p) and np.array_equal(s, want_s) and want_nts == st["n_nts_out"]
            assert st["n_solid"] == (st["n_nts_out"] - st["n_fragments"] * (k - 1)) + st["n_short"]
            if solid_min == 256:
                assert st["n_fragments"] == 0 and st["n_solid"] == 0 and st["n_slots"] > 0
                continue
            per_read = np.bincount(want["read"].astype(np.int64), minlength=n)
            assert (per_read >= 2).any() and (per_read == 0).any() and st["n_fragments"] > st["n_reads_kept"] > 0
            assert st["n_short"] > 0 or min_len == 0
            if min_len == 0:  # the first longest fragment of a read is what trim_reads keeps of it
                ivs = ix.trim_reads(seqs, solid_min)
                best = np.zeros(n, B.READ_INTERVAL_DTYPE)
                for f in want:
                    if f["len"] > best[int(f["read"])]["len"]:
                        best[int(f["read"])] = (f["start"], f["len"])
                assert np.array_equal(best, ivs)


@pytest.mark.parametrize("k,m,b", E2E_GEOMETRIES)
def test_recount_of_the_fragments(B, k, m, b):
    """index A from error-bearing reads; B counts the stream split_packed writes, C the fragments' strings: the same index"""
    seqs = error_reads(k)
    with B.BriskHip(k, m, b) as A, B.BriskHip(k, m, b) as ixb, B.BriskHip(k, m, b) as ixc:
        A.insert_reads(seqs)
        d_packed, d_starts, words, _ = device_reads(seqs)
        ask = SplitBuffers(0)  # the counters first: a call without room fills them
        st0 = A.split_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), 0, 0, ask.starts.data_ptr(), 0, 0, 2, 0, raise_on_capacity=False)
        assert st0.pop("rc") == ECAPACITY and ask.untouched()
        nf, need = st0["n_fragments"], (st0["n_nts_out"] + 15) // 16 + 2
        out = SplitBuffers(nf, need)
        st = A.split_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), out.packed.data_ptr(), need, out.starts.data_ptr(), 0, nf, 2, 0)
        assert (out.host()[2] == ROW_FILL).all()  # no table was asked for
        assert st["n_fragments"] > st["n_reads_kept"] and st["n_solid"] == st["n_nts_out"] - nf * (k - 1) and st["n_short"] == 0
        assert ixb.scan_bound(out.starts.data_ptr(), nf) == st["n_solid"]  # the k-mer instances of the stream: the solid ones, each once
        ixb.insert_packed(out.packed.data_ptr(), out.starts.data_ptr(), nf)
        rows, host_st = A.split_reads(seqs, 2, 0)
        assert host_st == st
        ixc.insert_reads([seqs[int(f["read"])][int(f["start"]):int(f["start"]) + int(f["len"])] for f in rows])
        got, want = ixb.checksum(), ixc.checksum()
    assert got == want and got[0] > 0, (k, got, want)


ENVIRONMENTS = {"whole": {}, "batch1": dict(BRISK_PROFILE_BATCH="1"), "batch5": dict(BRISK_PROFILE_BATCH="5")}
_outputs = {}


def outputs_of(name, tmp_path_factory):
    """the worker's bytes and stats in that environment (the library reads BRISK_PROFILE_BATCH once per process): run once, shared by the tests"""
    if name not in _outputs:
        path = str(tmp_path_factory.mktemp("split") / (name + ".pkl"))
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


@pytest.mark.parametrize("name", ("batch1", "batch5"))
def test_the_answer_does_not_depend_on_the_batches(B, name, tmp_path_factory):
    same_outputs(outputs_of(name, tmp_path_factory), outputs_of("whole", tmp_path_factory))


def test_the_answer_does_not_depend_on_max_batch_reads(B, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("split") / "max97.pkl")
    assert batches(path, 97) == 4
    with open(path, "rb") as f:
        same_outputs(pickle.load(f), outputs_of("whole", tmp_path_factory))


def test_deferred_inserts_and_refused_handles(B):
    rng = random.Random(7)
    reads = _random_reads(rng, 500, 2000)
    with B.BriskHip(63, 21, 14) as ix:  # two small insert calls: deferred until a call needs the index
        ix.insert_reads(reads[:250])
        ix.insert_reads(reads[250:])
        rows, st = ix.split_reads(reads, 1)
        assert rows.tolist() == [(r, 0, 150) for r in range(500)] and st["n_reads_kept"] == 500 and st["n_nts_out"] == st["n_nts_in"] == 75000
    with B.BriskHip(63, 21, 14) as ix:
        ix.insert_reads(reads[:250])
        ix.insert_reads(reads[250:])
        d_packed, d_starts, words, starts = device_reads(reads)
        out = SplitBuffers(500, len(words))
        st = ix.split_packed(d_packed.data_ptr(), d_starts.data_ptr(), 500, out.packed.data_ptr(), out.cap, out.starts.data_ptr(), out.frags.data_ptr(), 500, 1)
        assert st["n_fragments"] == 500 and np.array_equal(out.host()[0][:len(words)], words) and np.array_equal(out.host()[1][:501], starts)
        # refusals of the composed call leave the outputs as they were
        out = SplitBuffers(500, len(words))
        for cap_words, frag_cap in ((len(words) - 1, 500), (len(words), 499)):
            st2 = ix.split_packed(d_packed.data_ptr(), d_starts.data_ptr(), 500, out.packed.data_ptr(), cap_words, out.starts.data_ptr(), out.frags.data_ptr(), frag_cap, 1,
                                  raise_on_capacity=False)
            assert st2.pop("rc") == ECAPACITY and st2 == st and out.untouched()
        assert ix.L.brisk_hip_split_packed(ix.h, d_packed.data_ptr(), d_starts.data_ptr(), 500, 1, 0, None, 5, out.starts.data_ptr(), None, 500, C.byref(B.hipapi._SplitStats())) == EINVAL
        assert ix.L.brisk_hip_split_packed(ix.h, d_packed.data_ptr(), d_starts.data_ptr(), 500, 1, 0, None, 0, None, None, 500, C.byref(B.hipapi._SplitStats())) == EINVAL
        assert out.untouched()
    small = _random_reads(rng, 20, 500)
    for kw, word in ((dict(entry_ids=True), "entry-id"), (dict(n_owners=2, owner_rank=0), "sharded")):
        with B.BriskHip(31, 15, 14, **kw) as ix:
            with pytest.raises(B.BriskHipError) as e:
                ix.split_reads(small)
            assert e.value.code == EINVAL and word in str(e.value) and "split_reads" in str(e.value)
            d_packed, d_starts, words, _ = device_reads(small)
            out = SplitBuffers(20, len(words))
            with pytest.raises(B.BriskHipError) as e:
                ix.split_packed(d_packed.data_ptr(), d_starts.data_ptr(), 20, out.packed.data_ptr(), out.cap, out.starts.data_ptr(), out.frags.data_ptr(), 20)
            assert e.value.code == EINVAL and word in str(e.value) and "split_packed" in str(e.value) and out.untouched()
            # the run passes and the gather need no index
            assert check_fragment_gather(B, ix, small, [(r, r % 7, 150 - 2 * (r % 7) - r) for r in range(20)]) > 0
            slots = np.full(20 * 120, 0x103, np.uint16)
            slots[60::120] = 0x101
            d_slots, runs = to_device(slots), SplitBuffers(40)
            st = ix.solid_runs(d_slots.data_ptr(), d_starts.data_ptr(), 20, runs.frags.data_ptr(), 40, 2, 0)
            assert st["n_fragments"] == 40 and runs.rows(40).tolist() == [(r, s, n) for r in range(20) for s, n in ((0, 90), (61, 89))]


def test_brisk_count_rule_split(B, tmp_path):
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe):
        B.build_apps()
    fasta = os.path.join(ROOT, "tests", "golden", "test.fa")
    seqs = oracle.fasta_sequences(open(fasta).read())
    k, m, b = 31, 11, 4
    path = str(tmp_path / "fragments.fa")
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(seqs)
        some = False
        for solid, extra, min_len in ((1, [], 0), (2, ["--min-len", "40"], 40)):
            p = subprocess.run([exe, "--bulk", fasta, str(k), str(m), str(b), "--extract", path, "--rule", "split", "--solid", str(solid)] + extra, capture_output=True, text=True,
                               timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
            rows, st = B.fragments_from_slots(*ix.get_kmers(seqs), k, solid, min_len, n_nts_in=sum(len(s) for s in seqs))
            want = "".join(">%d %d %d\n%s\n" % (f["read"], f["start"], f["len"], seqs[int(f["read"])][int(f["start"]):int(f["start"]) + int(f["len"])]) for f in rows)
            assert open(path).read() == want, (solid, extra)
            assert "%d fragments of %d of %d reads, %d of %d nucleotides" % (st["n_fragments"], st["n_reads_kept"], st["n_reads"], st["n_nts_out"], st["n_nts_in"]) in p.stderr
            some |= len(rows) > 0
        assert some
    p = subprocess.run([exe, "--bulk", fasta, str(k), str(m), str(b), "--extract", path, "--rule", "splits"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 2 and "--rule: trim, median:LO:HI or present:LO:HI, got splits" in p.stderr  # a wrong rule exits as before
    p = subprocess.run([exe, "--bulk", fasta, str(k), str(m), str(b), "--extract", path, "--rule", "split", "--paired"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 2 and "--paired" in p.stderr
