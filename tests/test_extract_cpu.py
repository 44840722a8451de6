"""No GPU: the C-ABI of read extraction (five entry points, an interval, a rule), intervals_from_profile -- the rule's definition in
numpy -- on hand-made records with the answers written out, and the numpy extractor of extract_reference.py, which the GPU tests
trust, against plain Python string slicing and the library's host packer."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import brisk_amd
from brisk_amd import hipapi
from extract_reference import ascii_of, extract_reference, pack_codes, pack_reads, unpack_codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brisk_hip_select_intervals", "brisk_hip_extract_packed", "brisk_hip_trim_packed", "brisk_hip_trim_reads", "brisk_hip_unpack_ascii")
FIELDS = ("n_kmers", "n_present", "n_solid", "run_start", "run_len", "min_present", "max_present", "median", "median_present", "sum")


def test_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    L = C.CDLL(brisk_amd.build_library())
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in hipapi.SYMBOLS
        assert hasattr(L, s), s
        assert s in header.split("#ifndef BRISK_HIP_H")[0], s  # in the table of reference interfaces at the top
    L.brisk_hip_abi_version.restype = C.c_uint32
    assert L.brisk_hip_abi_version() == 4
    assert "#define BRISK_HIP_ABI_VERSION 4" in header
    for name in ("READ_INTERVAL_DTYPE", "select_rule", "intervals_from_profile", "SELECT_KINDS"):
        assert hasattr(brisk_amd, name), name
    for meth in ("trim_reads", "select_intervals", "extract_packed", "trim_packed", "unpack_ascii"):
        assert callable(getattr(brisk_amd.BriskHip, meth)), meth


def test_interval_and_rule_layout():
    dt = brisk_amd.READ_INTERVAL_DTYPE
    assert dt.itemsize == 8 and dt.names == ("start", "len") and [dt.fields[n][1] for n in dt.names] == [0, 4]
    header = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    assert "typedef struct brisk_hip_read_interval { uint32_t start, len; } brisk_hip_read_interval;" in header
    body = header[header.index("typedef struct brisk_hip_select_rule {"):header.index("} brisk_hip_select_rule;")]
    names = [n.strip() for m in re.finditer(r"^\s+uint32_t\s+([\w, ]+);", body, re.M) for n in m.group(1).split(",")]
    assert names == [n for n, _ in hipapi._SelectRule._fields_] == ["struct_size", "kind", "min_len", "lo", "hi"]
    assert C.sizeof(hipapi._SelectRule) == 20
    assert "enum { BRISK_HIP_SELECT_SOLID_RUN = 0, BRISK_HIP_SELECT_MEDIAN = 1, BRISK_HIP_SELECT_PRESENT = 2 };" in header
    assert brisk_amd.SELECT_KINDS == {"solid_run": 0, "trim": 0, "median": 1, "present": 2}
    r = brisk_amd.select_rule("median", 70, 1, 9)
    assert (r.struct_size, r.kind, r.min_len, r.lo, r.hi) == (20, 1, 70, 1, 9)
    r = brisk_amd.select_rule("solid_run")
    assert (r.kind, r.min_len, r.lo, r.hi) == (0, 0, 0, 0xffffffff)


def records(rows):
    """rows of (n_kmers, n_present, run_start, run_len, median)"""
    p = np.zeros(len(rows), brisk_amd.READ_PROFILE_DTYPE)
    for i, (n, present, start, run, med) in enumerate(rows):
        p[i]["n_kmers"], p[i]["n_present"], p[i]["run_start"], p[i]["run_len"], p[i]["median"] = n, present, start, run, med
        p[i]["n_solid"] = run
    return p


def iv(profile, k, rule):
    out = brisk_amd.intervals_from_profile(profile, k, rule)
    assert out.dtype == brisk_amd.READ_INTERVAL_DTYPE and len(out) == len(profile)
    return [(int(s), int(n)) for s, n in zip(out["start"], out["len"])]


def test_solid_run_rule():
    k = 31
    #            n_kmers present start run median
    p = records([(0, 0, 0, 0, 0),        # a read shorter than k
                 (120, 100, 0, 0, 1),    # no solid k-mer
                 (120, 100, 7, 1, 1),    # one solid k-mer: k nucleotides, the shortest interval there is
                 (120, 120, 0, 120, 3),  # the whole read
                 (120, 110, 50, 70, 3),  # a run that ends the read: [50, 50 + 70 + 30) = [50, 150)
                 (120, 90, 11, 40, 2)])
    assert iv(p, k, brisk_amd.select_rule("solid_run")) == [(0, 0), (0, 0), (7, 31), (0, 150), (50, 100), (11, 70)]
    # min_len: a run of 40 gives exactly 70 nucleotides -- kept at 70, dropped at 71; min_len below k means k
    assert iv(p, k, brisk_amd.select_rule("solid_run", min_len=70)) == [(0, 0), (0, 0), (0, 0), (0, 150), (50, 100), (11, 70)]
    assert iv(p, k, brisk_amd.select_rule("solid_run", min_len=71)) == [(0, 0), (0, 0), (0, 0), (0, 150), (50, 100), (0, 0)]
    assert iv(p, k, brisk_amd.select_rule("solid_run", min_len=5)) == iv(p, k, brisk_amd.select_rule("solid_run"))
    # one nucleotide fewer than min_len: run of 39 -> 69
    p = records([(120, 90, 11, 39, 2)])
    assert iv(p, k, brisk_amd.select_rule("solid_run", min_len=70)) == [(0, 0)]
    assert iv(p, k, brisk_amd.select_rule("solid_run", min_len=69)) == [(11, 69)]
    # lo and hi are not part of this rule
    assert iv(p, k, brisk_amd.select_rule("solid_run", lo=5, hi=6)) == [(11, 69)]
    assert len(brisk_amd.intervals_from_profile(records([]), k, brisk_amd.select_rule("solid_run"))) == 0


def test_median_rule():
    k = 63
    p = records([(0, 0, 0, 0, 5), (88, 88, 0, 88, 4), (88, 88, 0, 88, 5), (88, 88, 3, 20, 9), (88, 88, 0, 0, 10), (1, 1, 0, 1, 255), (38, 0, 0, 0, 0)])
    whole = [(0, 150), (0, 150), (0, 150), (0, 150), (0, 63), (0, 100)]  # of reads 1..6: the run does not matter
    assert iv(p, k, brisk_amd.select_rule("median", lo=5, hi=9)) == [(0, 0), (0, 0), whole[1], whole[2], (0, 0), (0, 0), (0, 0)]  # both edges are inside
    assert iv(p, k, brisk_amd.select_rule("median", lo=0, hi=4)) == [(0, 0), whole[0], (0, 0), (0, 0), (0, 0), (0, 0), whole[5]]
    assert iv(p, k, brisk_amd.select_rule("median", lo=255, hi=255)) == [(0, 0)] * 5 + [whole[4], (0, 0)]
    assert iv(p, k, brisk_amd.select_rule("median")) == [(0, 0)] + whole  # n_kmers == 0 is dropped whatever the bounds
    # min_len: the whole read has exactly n_kmers + k - 1 nucleotides
    assert iv(p, k, brisk_amd.select_rule("median", min_len=100)) == [(0, 0)] + whole[:4] + [(0, 0), whole[5]]
    assert iv(p, k, brisk_amd.select_rule("median", min_len=101)) == [(0, 0)] + whole[:4] + [(0, 0), (0, 0)]


def test_present_rule():
    k = 31
    #  permille of present k-mers: -, 1000, 0, 500, 499.x, 333.3, 1000
    p = records([(0, 0, 0, 0, 0), (120, 120, 0, 120, 2), (120, 0, 0, 0, 0), (120, 60, 0, 0, 0), (1201, 600, 0, 0, 0), (3, 1, 0, 0, 0), (1, 1, 0, 0, 1)])
    w = [(0, 150), (0, 150), (0, 150), (0, 1231), (0, 33), (0, 31)]
    assert iv(p, k, brisk_amd.select_rule("present", lo=1000, hi=1000)) == [(0, 0), w[0], (0, 0), (0, 0), (0, 0), (0, 0), w[5]]  # n_present == n_kmers
    assert iv(p, k, brisk_amd.select_rule("present", lo=0, hi=0)) == [(0, 0), (0, 0), w[1], (0, 0), (0, 0), (0, 0), (0, 0)]
    assert iv(p, k, brisk_amd.select_rule("present", lo=500, hi=1000)) == [(0, 0), w[0], (0, 0), w[2], (0, 0), (0, 0), w[5]]   # 600 / 1201 is below 500
    assert iv(p, k, brisk_amd.select_rule("present", lo=0, hi=500)) == [(0, 0), (0, 0), w[1], w[2], w[3], w[4], (0, 0)]
    assert iv(p, k, brisk_amd.select_rule("present", lo=333, hi=333)) == [(0, 0)] * 7   # 1 / 3 lies between 333 and 334
    assert iv(p, k, brisk_amd.select_rule("present", lo=333, hi=334)) == [(0, 0)] * 5 + [w[4], (0, 0)]
    assert iv(p, k, brisk_amd.select_rule("present")) == [(0, 0)] + w
    # products beyond 32 bits: 4e9 k-mers, permille bounds near 2^32
    big = records([(4_000_000_000, 4_000_000_000, 0, 0, 1), (4_000_000_000, 2_000_000_000, 0, 0, 1)])
    assert iv(big, k, brisk_amd.select_rule("present", lo=501, hi=0xffffffff)) == [(0, 4_000_000_030), (0, 0)]
    assert iv(big, k, brisk_amd.select_rule("present", lo=500, hi=500)) == [(0, 0), (0, 4_000_000_030)]


def test_an_interval_that_does_not_fit_32_bits_is_dropped():
    p = records([(0xffffffff, 0xffffffff, 0, 0xffffffff, 1), (0xffffffff - 62, 1, 0, 0xffffffff - 62, 1)])
    for kind in ("solid_run", "median", "present"):
        assert iv(p, 63, brisk_amd.select_rule(kind)) == [(0, 0), (0, 0xffffffff)]


def test_bad_rules_are_refused():
    p = records([(10, 10, 0, 10, 1)])
    for rule in (brisk_amd.select_rule(3), brisk_amd.select_rule("median", lo=2, hi=1), brisk_amd.select_rule("solid_run", lo=1, hi=0)):
        with pytest.raises(ValueError):
            brisk_amd.intervals_from_profile(p, 31, rule)
    short = brisk_amd.select_rule("median")
    short.struct_size = 16
    with pytest.raises(ValueError):
        brisk_amd.intervals_from_profile(p, 31, short)
    with pytest.raises(KeyError):
        brisk_amd.select_rule("mode")


def host_pack(lib, b):
    f = lib.brisk_hip_debug_host_pack
    f.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_int]
    f.restype = C.c_int
    out = np.zeros((len(b) + 15) // 16, np.uint32)
    assert f(b, len(b), out.ctypes.data, 0) == 0
    return out


def test_reference_extractor_against_string_slicing():
    lib = C.CDLL(brisk_amd.build_library())
    rng = random.Random(16)
    reads = ["".join(rng.choice("ACGT") for _ in range(rng.choice((1, 2, 15, 16, 17, 31, 32, 33, 100, 150, 200)))) for _ in range(400)]
    words, starts = pack_reads(reads)
    assert np.array_equal(words[:-2], host_pack(lib, "".join(reads).encode())) and not words[-2:].any()
    assert ascii_of(unpack_codes(words, int(starts[-1]))) == "".join(reads)
    for mode in ("mixed", "all", "none"):
        ivs = np.zeros(len(reads), brisk_amd.READ_INTERVAL_DTYPE)
        for i, r in enumerate(reads):
            if mode == "all" or (mode == "mixed" and rng.random() < 0.6):
                s = rng.randrange(len(r))
                ivs[i] = (s, rng.randint(1, len(r) - s))
        out, out_starts, out_index, n_out, n_nts = extract_reference(words, starts, ivs)
        kept = [(i, r[int(v["start"]):int(v["start"]) + int(v["len"])]) for i, (r, v) in enumerate(zip(reads, ivs)) if v["len"]]
        joined = "".join(s for _, s in kept)
        assert (n_out, n_nts) == (len(kept), len(joined)) and (mode != "mixed" or 0 < n_out < len(reads))
        assert out_index.tolist() == [i for i, _ in kept]
        assert out_starts.tolist() == [0] + np.cumsum([len(s) for _, s in kept]).tolist()
        assert len(out) == (n_nts + 15) // 16 + 2 and not out[-2:].any()
        assert np.array_equal(out[:-2], host_pack(lib, joined.encode()))  # (zero tail bits included: the host packer pads with zeros)
        for j in range(n_out):  # and read by read, through the output's own table
            a, b = int(out_starts[j]), int(out_starts[j + 1])
            assert ascii_of(unpack_codes(out, n_nts)[a:b]) == kept[j][1]
    out, out_starts, out_index, n_out, n_nts = extract_reference(np.zeros(2, np.uint32), np.zeros(1, np.uint64), np.zeros(0, brisk_amd.READ_INTERVAL_DTYPE))
    assert (n_out, n_nts, out.tolist(), out_starts.tolist(), len(out_index)) == (0, 0, [0, 0], [0], 0)
    assert np.array_equal(pack_codes([1, 2, 3]), np.array([(1 << 30) | (2 << 28) | (3 << 26)], np.uint32))


def test_brisk_count_knows_the_options():
    src = open(os.path.join(ROOT, "brisk_amd", "apps", "brisk_count.cpp")).read()
    assert '"--extract"' in src and '"--rule"' in src and '"--min-len"' in src and "brisk_hip_trim_reads(" in src
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe):
        brisk_amd.build_apps()
    usage = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--extract FILE --rule trim|median:LO:HI|present:LO:HI [--solid N] [--min-len L]" in usage


def test_extract_is_refused_outside_bulk_and_with_a_bad_rule(tmp_path):
    """no GPU needed: the refusals come before any device call"""
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe):
        brisk_amd.build_apps()
    fasta = os.path.join(ROOT, "tests", "golden", "test.fa")
    out = str(tmp_path / "kept.fa")
    for mode in ("--facade", "--mixed"):
        run = subprocess.run([exe, mode, fasta, "31", "11", "4", "--extract", out, "--rule", "trim"], capture_output=True, text=True, timeout=120)
        assert run.returncode == 2 and "--bulk only" in run.stderr, (run.returncode, run.stderr[-500:])
    for extra in (["--rule", "trim"], ["--min-len", "40"], ["--extract", out, "--rule", "mode:1:2"], ["--extract", out, "--rule", "median:3:2"],
                  ["--extract", out, "--rule", "median:1"], ["--extract", out, "--rule", "present:0:1000x"], ["--extract", out, "--min-len", "-1"], ["--extract"]):
        run = subprocess.run([exe, "--bulk", fasta, "31", "11", "4"] + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 2, (extra, run.returncode, run.stderr[-500:])
    assert not os.path.exists(out)


def test_the_feature_is_documented():
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "trim_packed" in readme and "--extract" in readme
    assert "Read extraction" in design and "brisk_hip_extract_packed" in design
