"""GPU: raw read intake.  brisk_hip_intake_ascii against the numpy definition (brisk_amd.fragments_from_reads) byte for byte --
packed words, the zero bits and the two zero words, the starts, the table, the stats, and the fill pattern behind every output --
then the host calls (intake, insert_raw) against insert_reads of the fragments' strings."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from extract_reference import pack_reads
from intake_reference import crafted_case, expected_outputs, fragment_strings, long_cases, most_fragments_in_a_word, quality_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "intake_worker.py")
EINVAL, ECAPACITY = 1, 5
FILL = 0xA5A5A5A5
ONES = np.uint64(2**64 - 1)


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


@pytest.fixture(scope="module")
def ix5(B):
    with B.BriskHip(5, 1, 1) as ix:
        yield ix


@pytest.fixture(scope="module")
def ix31(B):
    with B.BriskHip(31, 15, 14) as ix:
        yield ix


def to_device(raw):
    import torch
    t = torch.from_numpy(np.frombuffer(bytes(raw), np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


class Inputs:
    """reads on the device: the bytes sit `shift` (+ `first`) bytes into an allocation whose other bytes are valid bases of top quality,
    so that a kernel that looks outside [offsets[0], offsets[n]) finds fragments that the reference does not have"""

    def __init__(self, reads, quals=None, shift_b=0, shift_q=0, first=0):
        lens = [len(r) for r in reads]
        self.offsets = np.zeros(len(reads) + 1, np.uint64)
        self.offsets[1:] = np.cumsum(lens, dtype=np.uint64)
        self.offsets += np.uint64(first)
        self.n_bases = int(sum(lens))
        self.bases = to_device(b"A" * (16 + shift_b + first) + b"".join(reads) + b"C" * 80)
        self.p_bases = self.bases.data_ptr() + 16 + shift_b
        self.quals, self.p_quals = None, 0
        if quals is not None:
            self.quals = to_device(b"\xff" * (16 + shift_q + first) + b"".join(quals) + b"\xff" * 80)
            self.p_quals = self.quals.data_ptr() + 16 + shift_q
        self.d_offsets = to_device(self.offsets.tobytes())


class Outputs:
    def __init__(self, cap_words, frag_cap):
        import torch
        self.cap_words, self.frag_cap = cap_words, frag_cap
        self.packed = torch.full((cap_words + 8,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
        self.starts = torch.full((frag_cap + 1 + 4,), -1, dtype=torch.int64, device="cuda")
        self.frags = torch.full((2 * (frag_cap + 4),), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def host(self, B):
        return (self.packed.cpu().numpy().view(np.uint32), self.starts.cpu().numpy().view(np.uint64),
                self.frags.cpu().numpy().view(B.FRAGMENT_DTYPE))

    def untouched(self, B):
        w, s, f = self.host(B)
        return (w == FILL).all() and (s == ONES).all() and (f.view(np.uint64) == ONES).all()


def check_intake(B, ix, reads, quals=None, rule=None, shift_b=0, shift_q=0, first=0, tight=False, with_packed=True, with_frags=True, pass_quals=True):
    """one brisk_hip_intake_ascii call against the definition; returns (fragments, stats, expected starts)"""
    rule = B.intake_rule() if rule is None else rule
    L = max(rule.min_len, ix.k)
    want_frags, want_st = B.fragments_from_reads(reads, quals if rule.min_qual else None, ix.k, rule)
    want_words, want_starts = expected_outputs(reads, want_frags)
    assert np.array_equal(want_words, pack_reads([s.upper() for s in fragment_strings(reads, want_frags)], 2)[0])  # lower case packs as upper
    n, need = len(want_frags), len(want_words)
    assert need == (want_st["n_nts"] + 15) // 16 + 2
    inp = Inputs(reads, quals if pass_quals else None, shift_b, shift_q, first)
    # the room that always suffices, or exactly the room this case needs
    out = Outputs(need if tight else (inp.n_bases + 15) // 16 + 2, n if tight else inp.n_bases // L)
    st = ix.intake_ascii(inp.p_bases, inp.p_quals, inp.d_offsets.data_ptr(), len(reads), rule, out.packed.data_ptr() if with_packed else 0,
                         out.cap_words if with_packed else 0, out.starts.data_ptr(), out.frags.data_ptr() if with_frags else 0, out.frag_cap)
    assert st == want_st
    assert st["n_bases_in"] == st["n_nts"] + st["n_cut_base"] + st["n_cut_qual"] + st["n_short"]
    words, starts, frags = out.host(B)
    if with_packed:
        assert np.array_equal(words[:need], want_words)  # the used words, the zero bits that end the last one, the two zero words after
        assert (words[need:] == FILL).all()              # and nothing else
    else:
        assert (words == FILL).all()
    assert np.array_equal(starts[:n + 1], want_starts) and (starts[n + 1:] == ONES).all()
    if with_frags:
        assert np.array_equal(frags[:n], want_frags) and (frags[n:].view(np.uint64) == ONES).all()
    else:
        assert (frags.view(np.uint64) == ONES).all()
    return want_frags, st, want_starts


@pytest.mark.parametrize("L", [5, 31])
@pytest.mark.parametrize("variant", [0, 1])
def test_crafted_case(B, ix5, ix31, L, variant):
    ix = ix5 if L == 5 else ix31
    assert max(B.intake_rule().min_len, ix.k) == L
    reads, facts = crafted_case(L, variant)
    assert facts["run_align"] == {(n, a) for n in range(1, 41) for a in range(16)} and facts["boundary_align"] == set(range(16))
    assert facts["total"] % 16 and (facts["first_valid"], facts["last_valid"]) == ((True, False) if variant == 0 else (False, True))
    frags, st, starts = check_intake(B, ix, reads)
    assert L in frags["len"] and st["n_short"] > 0 and 0 < st["n_reads_kept"] < st["n_reads"] and facts["total"] > 2 * B.INTAKE_BLOCK
    if L == 5:
        assert most_fragments_in_a_word(starts) >= 4
    check_intake(B, ix, reads, tight=True)
    check_intake(B, ix, reads, with_frags=False)
    check_intake(B, ix, reads, with_packed=False)
    check_intake(B, ix, reads, first=3)            # offsets[0] != 0
    check_intake(B, ix, reads, rule=B.intake_rule(min_len=L + 4))


def test_all_valid_all_invalid_and_nothing(B, ix5):
    import random
    rng = random.Random(5)
    valid = ["".join(rng.choice("ACGTacgt") for _ in range(n)).encode() for n in (5, 16, 33, 1000, 7)]
    frags, st, _ = check_intake(B, ix5, valid)
    assert st["n_fragments"] == 5 and st["n_nts"] == st["n_bases_in"]
    frags, st, _ = check_intake(B, ix5, [b"NNNNNNNNNNNN", b"", b"\x00\xff" * 40, b"nnnn-\r\n"])
    assert st["n_fragments"] == 0 and st["n_cut_base"] == st["n_bases_in"]
    assert check_intake(B, ix5, [])[1]["n_reads"] == 0
    assert check_intake(B, ix5, [b"", b"", b""])[1]["n_bases_in"] == 0
    assert check_intake(B, ix5, [b"ACGT"])[1]["n_short"] == 4
    assert check_intake(B, ix5, [b"ACGTA"])[1]["n_fragments"] == 1


@pytest.mark.parametrize("L", [5, 31])
def test_long_runs(B, ix5, ix31, L):
    ix = ix5 if L == 5 else ix31
    for name, reads in long_cases(L, B.INTAKE_BLOCK).items():
        frags, st, _ = check_intake(B, ix, reads)
        if name.startswith("short"):
            assert st["n_short"] == L - 1 and st["n_fragments"] == 1 and int(frags["len"][0]) == 40 * B.INTAKE_BLOCK, name
        if name == "boundary_on_block":
            assert [int(n) for n in frags["len"]] == [B.INTAKE_BLOCK, 100]
        if name == "one_run":
            assert st["n_fragments"] == 1 and st["n_nts"] == 3 * B.INTAKE_BLOCK + 17
    check_intake(B, ix, long_cases(L, B.INTAKE_BLOCK)["short_read_after_40_blocks"], shift_b=5)  # blocks that do not start where the reads do


def test_displaced_inputs(B, ix5):
    seqs, quals = quality_case(60, 77, n_rate=0.05, read_len=40)
    rule = B.intake_rule(min_qual=20)
    for shift in range(16):
        check_intake(B, ix5, seqs, quals, rule, shift_b=shift, shift_q=shift)
    for sb in (0, 1, 15):
        for sq in (0, 1, 15):
            check_intake(B, ix5, seqs, quals, rule, shift_b=sb, shift_q=sq)


def test_quality(B, ix31, ix5):
    seqs, quals = quality_case(400, 3)
    frags, st, _ = check_intake(B, ix31, seqs, quals, B.intake_rule(min_qual=20))
    assert st["n_cut_base"] > 0 and st["n_cut_qual"] > 0 and st["n_short"] > 0 and st["n_fragments"] > 0
    check_intake(B, ix31, seqs, quals, B.intake_rule(min_qual=20, qual_base=0))
    q64 = [bytes(min(255, c + 31) for c in q) for q in quals]
    assert check_intake(B, ix31, seqs, q64, B.intake_rule(min_qual=20, qual_base=64))[1] == st
    check_intake(B, ix31, seqs, None, B.intake_rule())                    # no qualities at all
    plain = check_intake(B, ix31, seqs, quals, B.intake_rule())[1]       # qualities present, min_qual 0: ignored
    assert plain["n_cut_qual"] == 0 and plain["n_nts"] > st["n_nts"]
    # exactly at the threshold, one below, bytes above 127 (an unsigned compare), at both bases
    seq = b"ACGTACGTACGTACGTACGTACGTACGTACGT"
    for base in (33, 64):
        thr = base + 93
        qual = bytes([thr, thr - 1, thr + 1, 255, 128, 127, 0, thr] * 4)
        check_intake(B, ix5, [seq], [qual], B.intake_rule(min_len=1, min_qual=93, qual_base=base))
        check_intake(B, ix5, [seq], [qual], B.intake_rule(min_len=1, min_qual=1, qual_base=base))


def test_refusals(B, ix31):
    import ctypes as C
    seqs, quals = quality_case(50, 9)
    inp = Inputs(seqs, quals)
    frags, st = B.fragments_from_reads(seqs, None, 31)
    n, need = len(frags), (st["n_nts"] + 15) // 16 + 2
    out = Outputs(need, n)

    def call(rule, p_bases=inp.p_bases, p_quals=inp.p_quals, d_offsets=None, cap_words=need, frag_cap=n, p_starts=None, **kw):
        return ix31.intake_ascii(p_bases, p_quals, inp.d_offsets.data_ptr() if d_offsets is None else d_offsets, len(seqs), rule, out.packed.data_ptr(), cap_words,
                                 out.starts.data_ptr() if p_starts is None else p_starts, out.frags.data_ptr(), frag_cap, **kw)

    short = B.intake_rule()
    short.struct_size = 12
    bad = [(None, {}), (short, {}), (B.intake_rule(min_qual=94), {}), (B.intake_rule(qual_base=50), {}), (B.intake_rule(qual_base=1), {}),
           (B.intake_rule(min_qual=1), {"p_quals": 0}), (B.intake_rule(), {"p_bases": 0}), (B.intake_rule(), {"p_starts": 0})]
    down = inp.offsets.copy()
    down[7] = down[8] + np.uint64(1)
    d_down = to_device(down.tobytes())
    bad.append((B.intake_rule(), {"d_offsets": d_down.data_ptr()}))
    long_read = inp.offsets.copy()  # a read of 2^32 bytes: refused from the table alone, before a base is read
    long_read[-1] = long_read[-2] + np.uint64(2**32)
    d_long = to_device(long_read.tobytes())
    bad.append((B.intake_rule(), {"d_offsets": d_long.data_ptr()}))
    for rule, kw in bad:
        with pytest.raises(B.BriskHipError) as e:
            call(rule, **kw)
        assert e.value.code == EINVAL, (rule, kw)
        assert out.untouched(B)
    # the host calls check their table on the host, before anything is copied
    flat, rule, hst = np.frombuffer(b"".join(seqs), np.uint8).copy(), B.intake_rule(), B.hipapi._IntakeStats()
    rows = np.zeros(n + 1, B.FRAGMENT_DTYPE)
    for table in (down, long_read):
        assert ix31.L.brisk_hip_intake_reads(ix31.h, C.c_void_p(flat.ctypes.data), None, table, len(seqs), C.byref(rule), rows, n, C.byref(hst)) == EINVAL
        assert not rows.view(np.uint64).any()
        with B.BriskHip(31, 15, 14) as fresh:
            assert fresh.L.brisk_hip_insert_raw_reads(fresh.h, C.c_void_p(flat.ctypes.data), None, table, len(seqs), C.byref(rule), C.byref(hst)) == EINVAL
            assert fresh.stats()["nb_kmers"] == 0
    # the host table call with one row too few: ECAPACITY and the whole stats; with exactly the room: the table
    assert ix31.L.brisk_hip_intake_reads(ix31.h, C.c_void_p(flat.ctypes.data), None, inp.offsets, len(seqs), C.byref(rule), rows, n - 1, C.byref(hst)) == ECAPACITY
    assert hst.as_dict() == st
    assert ix31.L.brisk_hip_intake_reads(ix31.h, C.c_void_p(flat.ctypes.data), None, inp.offsets, len(seqs), C.byref(rule), rows, n, C.byref(hst)) == 0
    assert np.array_equal(rows[:n], frags) and hst.as_dict() == st
    with pytest.raises(B.BriskHipError) as e:  # a null offsets table
        ix31.intake_ascii(inp.p_bases, 0, 0, len(seqs), B.intake_rule(), out.packed.data_ptr(), need, out.starts.data_ptr(), 0, n)
    assert e.value.code == EINVAL
    # one too small: ECAPACITY, nothing written, the stats filled; then exactly that room
    for kw in ({"frag_cap": n - 1}, {"cap_words": need - 1}):
        with pytest.raises(B.BriskHipError) as e:
            call(B.intake_rule(), **kw)
        assert e.value.code == ECAPACITY
        got = call(B.intake_rule(), raise_on_capacity=False, **kw)
        assert got.pop("rc") == ECAPACITY and got == st and out.untouched(B)
    assert call(B.intake_rule()) == st and not out.untouched(B)
    check_intake(B, ix31, seqs, tight=True)
    check_intake(B, ix31, seqs, with_packed=False)  # d_out_packed == NULL: the table only


def period_fragments(B, buf, read_len, L):
    """fragments_from_reads of a buffer cut into reads of read_len bytes whose only non-bases are 'N', without a Python loop"""
    valid = buf != ord("N")
    at_read_start = np.zeros(len(buf), bool)
    at_read_start[::read_len] = True
    begins = np.nonzero(valid & (at_read_start | ~np.concatenate([[False], valid[:-1]])))[0]
    ends = np.nonzero(valid & np.concatenate([at_read_start[1:] | ~valid[1:], [True]]))[0] + 1
    lens = ends - begins
    keep = lens >= L
    frags = np.zeros(int(keep.sum()), B.FRAGMENT_DTYPE)
    frags["read"], frags["start"], frags["len"] = begins[keep] // read_len, begins[keep] % read_len, lens[keep]
    st = {"n_reads": len(buf) // read_len, "n_reads_kept": len(np.unique(frags["read"])), "n_fragments": len(frags), "n_bases_in": len(buf), "n_nts": int(lens[keep].sum()),
          "n_cut_base": int((~valid).sum()), "n_cut_qual": 0, "n_short": int(lens[~keep].sum())}
    return frags, st


def test_past_four_gigabytes(B, ix31):
    """4200 copies of a 1 MiB pattern: an N every 997 bytes of the pattern, a read boundary every 150 bytes of the buffer.  75
    patterns are a whole number of reads, so the fragment table repeats with that period: everything is checked in closed form from
    one period, and sampled fragments on both sides of byte 2^32 against the pattern."""
    import torch
    L, MIB, REPS, READ = 31, 1 << 20, 4200, 150
    rng = np.random.default_rng(12)
    pattern = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, MIB)].copy()
    pattern[::997] = ord("N")
    total = MIB * REPS
    period, reads_per_period = 75 * MIB, 75 * MIB // READ
    assert total > 2**32 + 2**26 and period % READ == 0 and REPS % 75 == 0
    n_reads = total // READ
    one = np.tile(pattern, 75)
    frags1, st1 = period_fragments(B, one, READ, L)
    head = B.fragments_from_reads([one[i * READ:(i + 1) * READ].tobytes() for i in range(2000)], None, L)[0]
    assert np.array_equal(frags1[:len(head)], head)  # the vectorised statement agrees with the definition where both are affordable
    n_periods = REPS // 75
    d_bases = torch.from_numpy(pattern).cuda().repeat(REPS)
    d_offsets = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * READ
    n_frag, n_nts = st1["n_fragments"] * n_periods, st1["n_nts"] * n_periods
    cap_words = (n_nts + 15) // 16 + 2
    d_packed = torch.empty(cap_words, dtype=torch.int32, device="cuda")
    d_starts = torch.empty(n_frag + 1, dtype=torch.int64, device="cuda")
    d_frags = torch.empty(2 * n_frag, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st = ix31.intake_ascii(d_bases.data_ptr(), 0, d_offsets.data_ptr(), n_reads, B.intake_rule(), d_packed.data_ptr(), cap_words, d_starts.data_ptr(), d_frags.data_ptr(), n_frag)
    assert st == {"n_reads": n_reads, **{f: st1[f] * n_periods for f in ("n_reads_kept", "n_fragments", "n_bases_in", "n_nts", "n_cut_base", "n_cut_qual", "n_short")}}
    assert st["n_bases_in"] == total == st["n_nts"] + st["n_cut_base"] + st["n_short"]
    # rows on both sides of the crossing, the first and the last
    starts1 = np.concatenate([[0], np.cumsum(frags1["len"].astype(np.int64))])
    src1 = frags1["read"].astype(np.int64) * READ + frags1["start"].astype(np.int64)
    p_cross = 2**32 // period
    j_cross = p_cross * len(frags1) + int(np.searchsorted(src1, 2**32 - p_cross * period))
    assert 0 < j_cross < n_frag
    rows = np.unique(np.concatenate([np.arange(0, 40), np.arange(j_cross - 60, j_cross + 60), np.arange(n_frag - 40, n_frag)]))
    idx = torch.from_numpy(rows).cuda()
    got_starts = d_starts[idx].cpu().numpy()
    got_rows = d_frags.view(-1, 2)[idx].cpu().numpy().copy().view(B.FRAGMENT_DTYPE).reshape(-1)
    assert int(d_starts[n_frag].item()) == n_nts
    below = above = 0
    out16 = torch.empty(4096, dtype=torch.uint8, device="cuda")
    for j, got_start, row in zip(rows, got_starts, got_rows):
        p, i = divmod(int(j), len(frags1))
        assert int(row["read"]) == int(frags1["read"][i]) + p * reads_per_period and int(row["start"]) == int(frags1["start"][i]) and int(row["len"]) == int(frags1["len"][i])
        assert int(got_start) == p * st1["n_nts"] + int(starts1[i])
        src = int(row["read"]) * READ + int(row["start"])
        below += src < 2**32
        above += src >= 2**32
        ix31.unpack_ascii(d_packed.data_ptr(), int(got_start), int(row["len"]), out16.data_ptr())
        torch.cuda.synchronize()
        want = np.take(pattern, np.arange(src, src + int(row["len"])) % MIB)  # (upper-case ACGT: what unpack_ascii spells)
        assert np.array_equal(out16[:int(row["len"])].cpu().numpy(), want)
    assert below > 50 and above > 50
    # the same bytes as ONE read: 2^32 - 1 bytes are the longest read the fragment record takes, 2^32 are refused (EINVAL, nothing
    # written).  Every run between two N of the pattern is a fragment (996 bytes, 728 at a pattern's end, 727 at this read's end).
    one_read = torch.tensor([0, 2**32 - 1], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st = ix31.intake_ascii(d_bases.data_ptr(), 0, one_read.data_ptr(), 1, B.intake_rule(), 0, 0, d_starts.data_ptr(), d_frags.data_ptr(), n_frag)
    n_cut = 4096 * len(range(0, MIB, 997))
    assert st == {"n_reads": 1, "n_reads_kept": 1, "n_fragments": n_cut, "n_bases_in": 2**32 - 1, "n_nts": 2**32 - 1 - n_cut, "n_cut_base": n_cut, "n_cut_qual": 0, "n_short": 0}
    last = d_frags.view(-1, 2)[n_cut - 1:n_cut].cpu().numpy().copy().view(B.FRAGMENT_DTYPE).reshape(-1)
    assert (int(last["read"][0]), int(last["start"][0]), int(last["len"][0])) == (0, 2**32 - 1 - 727, 727) and int(d_starts[n_cut].item()) == st["n_nts"]
    too_long = torch.tensor([0, 2**32], dtype=torch.int64, device="cuda")
    out = Outputs(16, 16)
    with pytest.raises(B.BriskHipError) as e:
        ix31.intake_ascii(d_bases.data_ptr(), 0, too_long.data_ptr(), 1, B.intake_rule(), out.packed.data_ptr(), out.cap_words, out.starts.data_ptr(), out.frags.data_ptr(), out.frag_cap)
    assert e.value.code == EINVAL and "2^32" in str(e.value) and out.untouched(B)


GEOMETRIES = [(63, 21, 14), (31, 15, 14), (31, 11, 4)]


def raw_body(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read().split(b"\n", 1)[1]  # the record's lines as they stand in the file, line ends included


def check_insert_raw(B, geo, seqs, quals=None, rule=None, calls=1, probe=False, **kw):
    rule = B.intake_rule() if rule is None else rule
    frags, want_st = B.fragments_from_reads(seqs, quals if rule.min_qual else None, geo[0], rule)
    strings = fragment_strings(seqs, frags)
    assert 0 < want_st["n_fragments"] and want_st["n_short"] > 0, "a case in which fragments are dropped"
    with B.BriskHip(*geo, **kw) as raw, B.BriskHip(*geo, **kw) as ref:
        got = dict.fromkeys(B.INTAKE_STATS_FIELDS, 0)
        step = (len(seqs) + calls - 1) // calls
        for c in range(0, len(seqs), step):
            st = raw.insert_raw(seqs[c:c + step], None if quals is None else quals[c:c + step], rule)
            got = {f: got[f] + st[f] for f in got}
        assert got == want_st
        ref.insert_reads(strings)
        if probe:  # the deferred insert is completed by the first call that needs the index
            assert np.array_equal(raw.get_reads(strings), ref.get_reads(strings))
            counts, found, base = raw.get_kmers(strings)
            assert found.all() and len(found) == int(base[-1]) > 0
        assert raw.checksum() == ref.checksum()
        assert raw.stats()["nb_kmers"] > 0


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_insert_raw_test_fa(B, geo):
    check_insert_raw(B, geo, [raw_body("test.fa")])


@pytest.mark.parametrize("geo", GEOMETRIES)
@pytest.mark.parametrize("min_qual", [0, 20])
def test_insert_raw_error_bearing_reads(B, geo, min_qual):
    seqs, quals = quality_case(2000, 11)
    check_insert_raw(B, geo, seqs, quals, B.intake_rule(min_qual=min_qual), probe=True)


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_insert_raw_variants(B, geo):
    seqs, quals = quality_case(2000, 12)
    rule = B.intake_rule(min_qual=20)
    check_insert_raw(B, geo, seqs, quals, rule, max_batch_reads=97)
    check_insert_raw(B, geo, seqs[:300], quals[:300], rule, calls=2, probe=True)  # two small calls: deferred
    check_insert_raw(B, geo, seqs, quals, rule, count_mode="saturate")
    check_insert_raw(B, geo, seqs * 3, quals * 3, rule, count_mode="saturate")


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_insert_raw_in_many_pieces(geo):
    env = dict(os.environ, BRISK_INTAKE_PIECE="300")
    r = subprocess.run([sys.executable, WORKER] + [str(v) for v in geo], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["equal"] and res["stats_equal"] and res["n_short"] > 0 and res["n_bases_in"] > 100 * 300


def test_intake_host_call(B, ix31):
    seqs, quals = quality_case(500, 21)
    for rule in (B.intake_rule(), B.intake_rule(min_qual=20), B.intake_rule(min_len=50, min_qual=10)):
        want, want_st = B.fragments_from_reads(seqs, quals, 31, rule)
        got, st = ix31.intake(seqs, quals, rule)
        assert np.array_equal(got, want) and st == want_st
    assert ix31.intake([s.decode() for s in seqs], None)[1] == B.fragments_from_reads(seqs, None, 31)[1]  # str
    with pytest.raises(ValueError):
        ix31.intake(seqs[:2], [quals[0], quals[1][:-1]], B.intake_rule(min_qual=20))
    with pytest.raises(ValueError):
        ix31.insert_raw(seqs[:2], [quals[0], quals[1][:-1]], B.intake_rule(min_qual=20))
    got, st = ix31.intake([], None)
    assert len(got) == 0 and st["n_reads"] == 0


@pytest.mark.parametrize("kw", [{"entry_ids": True}, {"n_owners": 2}])
def test_other_handles(B, kw):
    seqs, quals = quality_case(200, 31)
    rule = B.intake_rule(min_qual=20)
    with B.BriskHip(31, 15, 14, **kw) as ix:
        check_intake(B, ix, seqs, quals, rule)
        want, want_st = B.fragments_from_reads(seqs, quals, 31, rule)
        got, st = ix.intake(seqs, quals, rule)
        assert np.array_equal(got, want) and st == want_st
        with pytest.raises(B.BriskHipError) as raw:
            ix.insert_raw(seqs, quals, rule)
        with pytest.raises(B.BriskHipError) as clean:
            ix.insert_reads(fragment_strings(seqs, want))
        assert raw.value.code == clean.value.code == EINVAL and str(raw.value) == str(clean.value)


def write_fastq(path, seqs, quals, gz=False):
    import gzip
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(zip(seqs, quals)))
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(text)


def stats_line(stderr, path):
    lines = [l for l in stderr.splitlines() if l.startswith("fastq " + str(path) + ":")]
    assert len(lines) == 1, stderr
    return {kv.split("=")[0]: int(kv.split("=")[1]) for kv in lines[0].split(": ", 1)[1].split()}


def test_brisk_count_fastq(B, tmp_path):
    import oracle
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe):
        B.build_apps()
    k, m, b = 31, 15, 14
    seqs, quals = quality_case(1500, 41)
    other_s, other_q = quality_case(700, 42)
    fasta = os.path.join(GOLDEN, "test.fa")
    plain, gz, other = tmp_path / "reads.fq", tmp_path / "reads.fq.gz", tmp_path / "other.fq"
    write_fastq(plain, seqs, quals)
    write_fastq(gz, seqs, quals, gz=True)
    write_fastq(other, other_s, other_q)
    env = dict(os.environ, BRISK_BATCH_BASES="50000")  # several batches
    for min_qual in (0, 20):
        rule = B.intake_rule(min_qual=min_qual)
        with B.BriskHip(k, m, b) as ix:
            want_st = ix.insert_raw(seqs, quals, rule)
            assert want_st == B.fragments_from_reads(seqs, quals, k, rule)[1] and want_st["n_short"] > 0
            want = oracle.multiset_lines(*ix.enumerate(), k)
            ix.insert_raw(other_s, other_q, rule)
            want_merged = oracle.multiset_lines(*ix.enumerate(), k)
        for path in (plain, gz):
            dump = tmp_path / "dump.txt"
            p = subprocess.run([exe, "--bulk", str(path), str(k), str(m), str(b), str(dump), "--min-qual", str(min_qual)], capture_output=True, text=True, timeout=300, env=env)
            assert p.returncode == 0, p.stderr
            assert sorted(open(dump).read().splitlines()) == want
            assert stats_line(p.stderr, path) == want_st
        if min_qual == 0:  # the options may be left out
            p = subprocess.run([exe, "--bulk", str(plain), str(k), str(m), str(b), str(dump)], capture_output=True, text=True, timeout=300, env=env)
            assert p.returncode == 0 and sorted(open(dump).read().splitlines()) == want and stats_line(p.stderr, plain) == want_st, p.stderr
        if min_qual == 20:  # counts below 256 here: merging the second file's index is counting both files into one
            p = subprocess.run([exe, "--bulk", str(plain), str(k), str(m), str(b), str(dump), "--min-qual", "20", "--qual-base", "33", "--merge", str(other)], capture_output=True, text=True,
                               timeout=300, env=env)
            assert p.returncode == 0, p.stderr
            assert sorted(open(dump).read().splitlines()) == want_merged
            assert stats_line(p.stderr, other) == B.fragments_from_reads(other_s, other_q, k, rule)[1]
            # a FASTA main input with a FASTQ FILE takes the option too
            p = subprocess.run([exe, "--bulk", fasta, str(k), str(m), str(b), "-", "--min-qual", "20", "--merge", str(other)], capture_output=True, text=True, timeout=300, env=env)
            assert p.returncode == 0 and "fastq " + str(other) in p.stderr, p.stderr
    for args in ([fasta, "--min-qual", "20"], [fasta, "--qual-base", "64"], [str(plain), "--profile", str(tmp_path / "p.tsv")],
                 [str(plain), "--extract", str(tmp_path / "e.fa")], [str(plain), "--min-qual", "94"], [str(plain), "--qual-base", "50"]):
        p = subprocess.run([exe, "--bulk", args[0], str(k), str(m), str(b), "-"] + args[1:], capture_output=True, text=True, timeout=300)
        assert p.returncode == 2 and p.stderr.strip(), (args, p.stderr)
    p = subprocess.run([exe, "--facade", str(plain), str(k), str(m), str(b), "--min-qual", "20"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 2
    bad = tmp_path / "bad.fq"
    bad.write_bytes(b"@r0\nACGT\n+\nIII\n")
    p = subprocess.run([exe, "--bulk", str(bad), str(k), str(m), str(b), "-"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 1 and "FASTQ record 1" in p.stderr
