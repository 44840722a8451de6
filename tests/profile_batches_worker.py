"""Worker of test_profile_batches.py: one process per environment (the library reads BRISK_PROFILE_BATCH and BRISK_PROFILE_SEG once).
Fourteen reads as seven interleaved pairs through every call that walks a read stream in internal profile batches, each against the
numpy definitions; the refusals whose fault lies in a later batch.

    profile_batches_worker.py OUT     every output, by name, pickled into OUT: the test compares them across environments

Prints "ok <n checks>"."""
import ctypes as C
import os
import pickle
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["BRISK_INTAKE_PIECE"] = "500"  # read when a handle is created: clean_pairs (host) takes the 1336 bytes in three pieces
import numpy as np
import torch  # before the library: torch's HIP runtime first, as in the test process

import brisk_amd as B
from brisk_amd.hipapi import _host_ptr
from extract_reference import extract_reference, pack_reads
from extract_worker import FILL, OutBuffers, device_reads
from test_pairs import clean_route, filled_intervals, host_intervals, to_device, whole_reads

K, M, MB = 31, 11, 11  # one of test_extract.py's geometries
EINVAL = 1
SOLID = 2
COMP = str.maketrans("ACGT", "CATG")  # a substitution: never the same nucleotide
FAULT_ROW = 12  # the refusals' bad row: in the last batch under BRISK_PROFILE_BATCH = 1 and 5
OUTPUTS = {}


def keep(name, a):
    assert name not in OUTPUTS, name
    OUTPUTS[name] = np.ascontiguousarray(a).tobytes() if not isinstance(a, (bytes, str)) else a


def substitute(seq, positions):
    s = list(seq)
    for p in positions:
        s[p] = s[p].translate(COMP)
    return "".join(s)


def make_case():
    """(reads to index, the fourteen reads): every k-mer of the genome is solid, counts differ from place to place"""
    rng = random.Random(2323)
    genome = "".join(rng.choice("ACGT") for _ in range(2400))
    clean = [genome[p:p + 100] for p in (rng.randrange(0, 2300) for _ in range(300))] + [genome, genome]
    foreign = ["".join(rng.choice("ACGT") for _ in range(100)) for _ in range(2)]

    def g(at, n):
        return genome[at:at + n]

    reads = [g(10, 150), substitute(g(200, 150), [70]),       # pair 0: whole, cut
             "", g(400, 20),                                  # pair 1: empty; shorter than k, no slot
             g(500, K), substitute(g(600, 120), [30, 95]),    # pair 2: exactly k; a batch of five reads ends between these two
             g(800, 100), substitute(g(900, 200), [150]),     # pair 3: read 7 has 170 slots, three segments of 64, in the second batch of five
             foreign[0], g(1200, 90),                         # pair 4: the second mate alone
             substitute(g(1300, 180), [40]), g(1500, 60),     # pair 5
             g(1600, 35), foreign[1]]                         # pair 6: the first mate alone
    assert len(reads) == 14 and len(reads[7]) - K + 1 > 2 * 64
    return clean, reads


def make_raw(reads):
    """the same reads as raw bytes with qualities: N, another byte, lower case, one base of low quality"""
    raw = [bytearray(r.encode()) for r in reads]
    raw[0][60] = ord("N")                       # fragments of 60 and 89: the second is the longest
    raw[1][20:50] = bytes(raw[1][20:50]).lower()
    raw[6][50] = ord("N")                       # fragments of 50 and 49
    raw[7][10] = ord("-")                       # a fragment shorter than k, then 189
    quals = [bytearray(b"I" * len(r)) for r in raw]
    quals[10][100] = ord("#")                   # Phred 2: cut like an N
    return [bytes(r) for r in raw], [bytes(q) for q in quals]


def unpacked(ix, d_stream, n_nts):
    if not n_nts:
        return ""
    d = torch.zeros(n_nts, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ix.unpack_ascii(d_stream.data_ptr(), 0, n_nts, d.data_ptr())
    ix.sync()
    return d.cpu().numpy().tobytes().decode()


def check_stream(out, want, what):
    """one output stream against extract_reference's (words, starts, index, n, nts): the used words and nothing else"""
    w_words, w_starts, w_index, w_n, _ = want
    got, got_starts, got_index = out.host()
    assert np.array_equal(got[:len(w_words)], w_words) and (got[len(w_words):] == FILL).all(), what
    assert np.array_equal(got_starts[:w_n + 1], w_starts) and (got_starts[w_n + 1:] == np.uint64(2**64 - 1)).all(), what
    assert np.array_equal(got_index[:w_n], w_index) and (got_index[w_n:] == np.uint64(2**64 - 1)).all(), what
    return got[:len(w_words)], got_starts[:w_n + 1], got_index[:w_n]


def two_outs(n, cap):
    outs = [OutBuffers(n, cap), OutBuffers(n, cap)]
    return outs, [(o.packed.data_ptr(), o.cap, o.starts.data_ptr(), o.index.data_ptr()) for o in outs]


def profiles_and_trims(ix, reads):
    n = len(reads)
    checks = 0
    slots = ix.get_kmers(reads)
    d_packed, d_starts, words, starts = device_reads(reads)
    for s in (1, SOLID, 9):
        want = B.profile_from_slots(*slots, s)
        got = ix.read_profile(reads, s)
        assert np.array_equal(got, want), ("read_profile", s, got, want)
        d_out = torch.full((n * 32,), 0x77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ix.read_profile_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, d_out.data_ptr(), s)
        got_p = d_out.cpu().numpy().view(B.READ_PROFILE_DTYPE)
        assert np.array_equal(got_p, want), ("read_profile_packed", s, got_p, want)
        keep("profile/%d" % s, got)
        keep("profile_packed/%d" % s, got_p)
        checks += 2
    prof = B.profile_from_slots(*slots, SOLID)
    assert prof["n_kmers"][2] == 0 and prof["n_kmers"][3] == 0 and prof["n_kmers"][4] == 1 and prof["n_kmers"][7] == 170
    assert (prof["run_len"] < prof["n_kmers"]).sum() >= 4 and len(np.unique(prof["median"])) >= 4
    rules = {"solid_run": B.select_rule("solid_run"), "median": B.select_rule("median", lo=int(np.median(prof["median"])) + 1, hi=255, min_len=40)}
    for name, rule in rules.items():
        want_iv = B.intervals_from_profile(prof, K, rule)
        assert 0 < (want_iv["len"] > 0).sum() < n, name
        got_iv = ix.trim_reads(reads, SOLID, rule)
        assert np.array_equal(got_iv, want_iv), ("trim_reads", name, got_iv, want_iv)
        want = extract_reference(words, starts, want_iv)
        out = OutBuffers(n, len(words))
        got_n = ix.trim_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, out.packed.data_ptr(), out.cap, out.starts.data_ptr(), out.index.data_ptr(), SOLID, rule)
        assert got_n == (want[3], want[4]), ("trim_packed", name, got_n)
        stream = check_stream(out, want, ("trim_packed", name))
        bases = unpacked(ix, out.packed, got_n[1])
        assert bases == "".join(r[int(v["start"]):int(v["start"]) + int(v["len"])] for r, v in zip(reads, want_iv)), ("trim_packed", name, "bases")
        keep("trim_reads/" + name, got_iv)
        for part, a in zip(("words", "starts", "index"), stream):
            keep("trim_packed/%s/%s" % (name, part), a)
        keep("trim_packed/%s/bases" % name, bases)
        checks += 2
    cut = B.intervals_from_profile(prof, K, rules["solid_run"])
    assert ((cut["len"] > 0) & (cut["len"] < [len(r) for r in reads])).sum() >= 4, "the rule cuts inside no read"
    return prof, rules["solid_run"], checks


def trim_pairs(ix, reads, prof, rule):
    n = len(reads)
    checks = 0
    d_packed, d_starts, words, starts = device_reads(reads)
    each = B.intervals_from_profile(prof, K, rule)
    whole = whole_reads(B, prof, K, rule.min_len)
    c = B.split_pairs(each)[2]
    assert min(c["n_pairs_kept"], c["n_single_first"], c["n_single_second"], c["n_pairs_dropped"]) >= 1, c
    for mode in ("each", "all", "any"):
        final = B.pair_intervals(each, whole, mode)
        iv_p, iv_s, counts = B.split_pairs(final)
        want = [extract_reference(words, starts, t) for t in (iv_p, iv_s)]
        got_iv, got_counts = ix.trim_pairs(reads, None, SOLID, rule, mode)
        assert np.array_equal(got_iv, final), ("trim_pairs", mode, got_iv, final)
        assert got_counts == counts, ("trim_pairs", mode, got_counts, counts)     # all eight
        outs, args = two_outs(n, len(words))
        got_counts = ix.trim_pairs_packed(d_packed.data_ptr(), d_starts.data_ptr(), n, args[0], args[1], SOLID, rule, mode)
        assert got_counts == counts, ("trim_pairs_packed", mode, got_counts, counts)
        keep("trim_pairs/%s/intervals" % mode, got_iv)
        keep("trim_pairs/%s/counts" % mode, repr(sorted(got_counts.items())))
        for which, o, w in zip(("pairs", "singles"), outs, want):
            for part, a in zip(("words", "starts", "index"), check_stream(o, w, ("trim_pairs_packed", mode, which))):
                keep("trim_pairs_packed/%s/%s/%s" % (mode, which, part), a)
        if mode == "any":
            assert (final["len"] > each["len"]).any(), "no mate was restored whole"
        checks += 2
    return checks


def clean_pairs(ix, raw, quals):
    n = len(raw)
    checks = 0
    intake = B.intake_rule(min_qual=10)
    rule = B.select_rule("solid_run")
    flat = np.frombuffer(b"".join(raw), np.uint8).copy()
    qflat = np.frombuffer(b"".join(quals), np.uint8).copy()
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in raw])
    words, starts = pack_reads(raw)
    d_bases, d_quals, d_offs = to_device(flat), to_device(qflat), to_device(offs)
    for mode in ("each", "all", "any"):
        final, each, iv1, stats = clean_route(B, ix, raw, quals, K, intake, rule, SOLID, mode)
        assert (iv1["len"] > 0).sum() > 5 and ((each["len"] > 0) & (each["len"] < iv1["len"])).sum() >= 2 and stats["n_cut_qual"] == 1 and stats["n_short"] >= 1
        iv_p, iv_s, counts = B.split_pairs(final)
        want = [extract_reference(words, starts, t) for t in (iv_p, iv_s)]
        outs, args = two_outs(n, len(words))
        d_iv = filled_intervals(n)
        got_counts, got_stats = ix.clean_pairs_ascii(d_bases.data_ptr(), d_quals.data_ptr(), d_offs.data_ptr(), n, intake, args[0], args[1], rule, SOLID, mode, d_iv.data_ptr())
        assert got_counts == counts and got_stats == stats, ("clean_pairs_ascii", mode, got_counts, counts, got_stats, stats)
        got_iv, clean = host_intervals(B, d_iv, n)
        assert np.array_equal(got_iv, final) and clean, ("clean_pairs_ascii", mode, got_iv, final)
        keep("clean_pairs_ascii/%s/intervals" % mode, got_iv)
        for which, o, w in zip(("pairs", "singles"), outs, want):
            for part, a in zip(("words", "starts", "index"), check_stream(o, w, ("clean_pairs_ascii", mode, which))):
                keep("clean_pairs_ascii/%s/%s/%s" % (mode, which, part), a)
        got_iv, got_counts, got_stats = ix.clean_pairs(raw, None, quals, None, intake, rule, SOLID, mode)   # (three pieces of whole pairs)
        assert np.array_equal(got_iv, final) and got_counts == counts and got_stats == stats, ("clean_pairs", mode, got_iv, final, got_counts, counts, got_stats, stats)
        keep("clean_pairs/%s/intervals" % mode, got_iv)
        keep("clean_pairs/%s/counts" % mode, repr((sorted(got_counts.items()), sorted(got_stats.items()))))
        checks += 2
    c = B.split_pairs(clean_route(B, ix, raw, quals, K, intake, rule, SOLID, "each")[0])[2]
    assert min(c["n_pairs_kept"], c["n_single_first"], c["n_single_second"], c["n_pairs_dropped"]) >= 1, c
    return checks


def refusals(ix, reads, raw, quals):
    n = len(reads)
    checks = 0
    batch = int(os.environ.get("BRISK_PROFILE_BATCH", "0")) or n
    rule, intake = B.select_rule("solid_run"), B.intake_rule(min_qual=10)

    def last_error():
        return ix.L.brisk_hip_last_error(ix.h).decode()

    # the packed calls: a read table that does not ascend at FAULT_ROW
    d_packed, d_starts, words, starts = device_reads(reads)
    bad = np.array(starts)
    bad[FAULT_ROW], bad[FAULT_ROW + 1] = starts[FAULT_ROW + 1], starts[FAULT_ROW]
    d_bad = to_device(bad)
    d_out = torch.full((n * 32,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ix.L.brisk_hip_read_profile_packed(ix.h, d_packed.data_ptr(), d_bad.data_ptr(), n, SOLID, d_out.data_ptr()) == EINVAL and "ascend" in last_error(), last_error()
    torch.cuda.synchronize()
    # (the records of the batches before the faulty one are out: the header promises "nothing written" for the streams, not for these)
    assert (d_out.cpu().numpy()[FAULT_ROW // batch * batch * 32:] == 0x77).all(), "read_profile_packed wrote the faulty batch's records"
    out = OutBuffers(n, len(words))
    n1, n2 = C.c_uint64(77), C.c_uint64(77)
    assert ix.L.brisk_hip_trim_packed(ix.h, d_packed.data_ptr(), d_bad.data_ptr(), n, SOLID, C.byref(rule), out.packed.data_ptr(), out.cap, out.starts.data_ptr(),
                                      out.index.data_ptr(), C.byref(n1), C.byref(n2)) == EINVAL and "ascend" in last_error(), last_error()
    assert out.untouched(), "a refused trim_packed wrote to its output"
    for mode in ("each", "any"):
        outs, args = two_outs(n, len(words))
        try:
            ix.trim_pairs_packed(d_packed.data_ptr(), d_bad.data_ptr(), n, args[0], args[1], SOLID, rule, mode)
            raise AssertionError("trim_pairs_packed took a table that does not ascend")
        except B.BriskHipError as e:
            assert e.code == EINVAL and "ascend" in str(e), str(e)
        assert outs[0].untouched() and outs[1].untouched(), "a refused trim_pairs_packed wrote to an output"
    flat = np.frombuffer(b"".join(raw), np.uint8).copy()
    qflat = np.frombuffer(b"".join(quals), np.uint8).copy()
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in raw])
    bad = offs.copy()
    bad[FAULT_ROW], bad[FAULT_ROW + 1] = offs[FAULT_ROW + 1], offs[FAULT_ROW]
    d_bases, d_quals, d_offs = to_device(flat), to_device(qflat), to_device(bad)
    outs, args = two_outs(n, len(flat) // 16 + 3)
    d_iv = filled_intervals(n)
    try:
        ix.clean_pairs_ascii(d_bases.data_ptr(), d_quals.data_ptr(), d_offs.data_ptr(), n, intake, args[0], args[1], rule, SOLID, "each", d_iv.data_ptr())
        raise AssertionError("clean_pairs_ascii took a table that does not ascend")
    except B.BriskHipError as e:
        assert e.code == EINVAL and "ascend" in str(e), str(e)
    assert outs[0].untouched() and outs[1].untouched() and host_intervals(B, d_iv, 0)[1], "a refused clean_pairs_ascii wrote to an output"
    checks += 5

    # the host calls: read FAULT_ROW + 1 is too long for the record (refused from the table alone, before a base is read)
    flat_r = np.frombuffer("".join(reads).encode(), np.uint8).copy()
    long_r = np.zeros(n + 1, np.uint64)
    long_r[1:] = np.cumsum([len(s) for s in reads])
    long_r[n] = long_r[n - 1] + np.uint64(2**32 + 100)
    long_raw = offs.copy()
    long_raw[n] = long_raw[n - 1] + np.uint64(2**32 + 100)

    def refused(rc, who, *outputs):
        assert rc == EINVAL and last_error().startswith(who + ": a read of ") and "2^32" in last_error() and "does not fit" in last_error(), (who, rc, last_error())
        for o in outputs:
            assert (np.frombuffer(bytes(o), np.uint8) == 0x77).all(), who + ": a refused call wrote to its output"

    def filled(dtype_or_struct):
        if isinstance(dtype_or_struct, np.dtype):
            return np.frombuffer(b"\x77" * (n * dtype_or_struct.itemsize), dtype_or_struct).copy()
        o = dtype_or_struct()
        C.memset(C.byref(o), 0x77, C.sizeof(o))
        return o

    out = filled(B.READ_PROFILE_DTYPE)
    refused(ix.L.brisk_hip_read_profile_reads(ix.h, flat_r, long_r, n, SOLID, out), "read_profile", out.tobytes())
    out = filled(B.READ_INTERVAL_DTYPE)
    refused(ix.L.brisk_hip_trim_reads(ix.h, flat_r, long_r, n, SOLID, C.byref(rule), out), "trim_reads", out.tobytes())
    for mode in (0, 2):
        out, pc = filled(B.READ_INTERVAL_DTYPE), filled(B.hipapi._PairCounts)
        refused(ix.L.brisk_hip_trim_pairs_reads(ix.h, flat_r, long_r, n, SOLID, C.byref(rule), mode, out, C.byref(pc)), "trim_pairs_reads", out.tobytes(), pc)
    out, pc, st = filled(B.READ_INTERVAL_DTYPE), filled(B.hipapi._PairCounts), filled(B.hipapi._IntakeStats)
    refused(ix.L.brisk_hip_clean_pairs_reads(ix.h, _host_ptr(flat), _host_ptr(qflat), long_raw, n, C.byref(intake), C.byref(rule), SOLID, 0, out, C.byref(pc), C.byref(st)),
            "clean_pairs_reads", out.tobytes(), pc, st)
    checks += 5
    # the handle is as it was
    assert np.array_equal(ix.read_profile(reads, SOLID), B.profile_from_slots(*ix.get_kmers(reads), SOLID))
    return checks


def main(out_path):
    assert torch.cuda.is_available()
    clean, reads = make_case()
    raw, quals = make_raw(reads)
    with B.BriskHip(K, M, MB) as ix:
        ix.insert_reads(clean)
        prof, rule, checks = profiles_and_trims(ix, reads)
        checks += trim_pairs(ix, reads, prof, rule)
        checks += clean_pairs(ix, raw, quals)
        checks += refusals(ix, reads, raw, quals)
    with open(out_path, "wb") as f:
        pickle.dump(OUTPUTS, f)
    print(f"ok {checks}")


if __name__ == "__main__":
    main(sys.argv[1])
