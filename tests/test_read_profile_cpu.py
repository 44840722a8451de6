"""No GPU: the C-ABI of the per-read abundance profile (two entry points, one 32-byte record) and profile_from_slots, the
record's definition in plain numpy, on hand-written slots with the answers written out."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

import brisk_amd
from brisk_amd import hipapi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brisk_hip_read_profile_reads", "brisk_hip_read_profile_packed")
FIELDS = ("n_kmers", "n_present", "n_solid", "run_start", "run_len", "min_present", "max_present", "median", "median_present", "sum")


def test_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    lib = brisk_amd.build_library()
    L = C.CDLL(lib)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in hipapi.SYMBOLS
        assert hasattr(L, s), s
    L.brisk_hip_abi_version.restype = C.c_uint32
    assert L.brisk_hip_abi_version() == 4
    assert "#define BRISK_HIP_ABI_VERSION 4" in header
    # both are in the table of reference interfaces at the top
    assert "brisk_hip_read_profile_reads / brisk_hip_read_profile_packed" in header.split("#ifndef BRISK_HIP_H")[0]


def test_record_layout():
    dt = brisk_amd.READ_PROFILE_DTYPE
    assert dt.itemsize == 32
    assert dt.names == FIELDS
    assert [dt.fields[n][1] for n in FIELDS] == [0, 4, 8, 12, 16, 20, 21, 22, 23, 24]
    # the header's struct, compiled, has the same layout
    header = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    body = header[header.index("typedef struct brisk_hip_read_profile {"):header.index("} brisk_hip_read_profile;")]
    assert [m.group(1) for m in re.finditer(r"^\s+uint\d+_t\s+(\w+);", body, re.M)] == list(FIELDS)


def prof(slots_per_read, solid_min):
    """slots_per_read: one list per read of None (absent) or a count"""
    counts, found, base = [], [], [0]
    for read in slots_per_read:
        counts += [0 if v is None else v for v in read]
        found += [v is not None for v in read]
        base.append(len(counts))
    return brisk_amd.profile_from_slots(np.array(counts, np.uint8), np.array(found, bool), np.array(base, np.uint64), solid_min)


def rec(p):
    return tuple(int(p[f]) for f in FIELDS)


def test_empty_one_slot_absent_and_solid_reads():
    _ = None
    p = prof([[], [5], [_], [_, _, _], [3, 3, 3, 3]], 2)
    assert p.dtype == brisk_amd.READ_PROFILE_DTYPE and len(p) == 5
    #                 n  pres solid start len min max med medp sum
    assert rec(p[0]) == (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert rec(p[1]) == (1, 1, 1, 0, 1, 5, 5, 5, 5, 5)
    assert rec(p[2]) == (1, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert rec(p[3]) == (3, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert rec(p[4]) == (4, 4, 4, 0, 4, 3, 3, 3, 3, 12)
    assert len(prof([], 2)) == 0


def test_lower_medians_even_and_odd():
    _ = None
    # even n: sorted all-slots [0, 0, 1, 4, 7, 9] -> index 2; present [1, 4, 7, 9] -> index 1
    p = prof([[9, _, 1, 7, _, 4]], 1)
    assert rec(p[0]) == (6, 4, 4, 2, 2, 1, 9, 1, 4, 21)
    # odd n: sorted all-slots [0, 2, 5, 8, 8] -> index 2; present [2, 5, 8, 8] -> index 1
    p = prof([[8, 2, _, 8, 5]], 1)
    assert rec(p[0]) == (5, 4, 4, 0, 2, 2, 8, 5, 5, 23)
    # odd number of present slots: [2, 6, 10] -> 6; all [0, 0, 0, 2, 6, 10] -> index 2 -> 0
    p = prof([[_, 10, _, 2, 6, _]], 1)
    assert rec(p[0]) == (6, 3, 3, 3, 2, 2, 10, 0, 6, 18)


def test_a_present_slot_of_count_zero():
    """a count that wrapped to 0: present, solid only when solid_min is 0"""
    _ = None
    reads = [[0], [4, 0, 4, _]]
    p0, p1 = prof(reads, 0), prof(reads, 1)
    assert rec(p0[0]) == (1, 1, 1, 0, 1, 0, 0, 0, 0, 0)
    assert rec(p1[0]) == (1, 1, 0, 0, 0, 0, 0, 0, 0, 0)
    assert rec(p0[1]) == (4, 3, 3, 0, 3, 0, 4, 0, 4, 8)
    assert rec(p1[1]) == (4, 3, 2, 0, 1, 0, 4, 0, 4, 8)


def test_runs_first_of_equal_and_one_that_ends_the_read():
    _ = None
    # two runs of three: the first wins
    p = prof([[1, 5, 5, 5, 1, _, 6, 6, 6, 1]], 2)
    assert rec(p[0]) == (10, 9, 6, 1, 3, 1, 6, 5, 5, 36)
    # the longest run ends at the last slot
    p = prof([[7, 7, _, 7, 7, 7]], 2)
    assert rec(p[0]) == (6, 5, 5, 3, 3, 7, 7, 7, 7, 35)
    # solid_min decides what a run is
    p = prof([[2, 3, 3, 2, 2, 2]], 3)
    assert rec(p[0]) == (6, 6, 2, 1, 2, 2, 3, 2, 2, 14)


def test_solid_min_256_and_counts_of_255():
    p = prof([[255, 255, 255], [255, None]], 255)
    assert rec(p[0]) == (3, 3, 3, 0, 3, 255, 255, 255, 255, 765)
    assert rec(p[1]) == (2, 1, 1, 0, 1, 255, 255, 0, 255, 255)
    p = prof([[255, 255, 255], [255, None]], 256)
    assert rec(p[0]) == (3, 3, 0, 0, 0, 255, 255, 255, 255, 765)
    assert rec(p[1]) == (2, 1, 0, 0, 0, 255, 255, 0, 255, 255)


def test_several_reads_use_their_own_slots():
    _ = None
    p = prof([[4, 4], [], [_, 9, 9, 9], [1]], 2)
    assert [rec(x) for x in p] == [(2, 2, 2, 0, 2, 4, 4, 4, 4, 8), (0,) * 10, (4, 3, 3, 1, 3, 9, 9, 9, 9, 27), (1, 1, 0, 0, 0, 1, 1, 1, 1, 1)]


def test_brisk_count_knows_the_options():
    src = open(os.path.join(ROOT, "brisk_amd", "apps", "brisk_count.cpp")).read()
    assert '"--profile"' in src and '"--solid"' in src and "brisk_hip_read_profile_reads(" in src


def test_profile_is_refused_outside_bulk(tmp_path):
    """no GPU needed: the refusal comes before any device call"""
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe):
        brisk_amd.build_apps()
    fasta = os.path.join(ROOT, "tests", "golden", "test.fa")
    out = str(tmp_path / "p.tsv")
    for mode in ("--facade", "--mixed"):
        for extra in (["--profile", out], ["--profile", out, "--solid", "3"]):
            run = subprocess.run([exe, mode, fasta, "31", "11", "4"] + extra, capture_output=True, text=True, timeout=120)
            assert run.returncode == 2 and "--bulk only" in run.stderr, (run.returncode, run.stderr[-500:])
    for extra in (["--solid", "3"], ["--profile", out, "--solid", "x"], ["--profile"]):
        run = subprocess.run([exe, "--bulk", fasta, "31", "11", "4"] + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 2, (extra, run.returncode, run.stderr[-500:])
    assert not os.path.exists(out)


def test_the_environment_knob_is_documented():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "BRISK_PROFILE_SEG" in readme and "read_profile" in readme
