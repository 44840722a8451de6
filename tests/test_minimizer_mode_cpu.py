"""CPU-side checks of full-width minimizers (brisk_hip_options.minimizer_mode).  The yardstick of full mode is the restatement of the
enumerator in tests/minimizer_reference.py: here it is held against the oracle (and the reference build, where there is one) in
reference mode, shown to be the same function in both modes where k <= 32, and shown to give one identity per canonical k-mer in
full mode at k > 32 where the reference's truncation gives several.  Then the boundary: header, enum, ctypes structures, snapshot
byte 116, brisk_count's usage text.  No device is needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import brisk_amd
import minimizer_reference as MR
import oracle
from brisk_amd import hipapi
from snapshot_reader import pack_header, block_bytes

GEOMETRIES = [(k, m) for k in (31, 32, 33, 34, 47, 63) for m in (3, 11, 15, 21, 31) if m < k]
EFORMAT = 8
FIELDS = dict(version=1, header_bytes=256, k=63, m=21, b=14, data_bytes=1, part_bits=24, ext_bits=0, cls_bits=0, cls_width=1, key_words=2, shift=4,
              n_entries=5, n_partitions=2, nb_skmers=77, checksum=(5, 9, 0x0123456789ABCDEF), n_blocks=1)


def as_enumerated(res):
    skm_ret, skm_n, lo, hi, idx, _ = res
    return [(int(a), int(b), int(c)) for a, b, c in zip(lo, hi, idx)], [int(x) for x in skm_n], [int(x) for x in skm_ret]


@pytest.fixture(scope="module")
def O():
    return MR.the_oracle()


@pytest.fixture(scope="module")
def lib():
    brisk_amd.build_library()
    return hipapi.load()


@pytest.mark.parametrize("k,m", GEOMETRIES)
def test_the_restatement_is_the_oracle_in_reference_mode(O, k, m):
    ref = oracle.Ref() if oracle.have_ref() else None
    for r in MR.parity_reads():
        if len(r) < k:
            continue
        got = MR.enumerate_read(r, k, m, full=False)
        assert (got.kmers, got.cuts, got.rets) == as_enumerated(O.enumerate(r, k, m)), (k, m, r)
        if ref is not None:
            assert (got.kmers, got.cuts, got.rets) == as_enumerated(ref.enumerate(r, k, m)), (k, m, r)


@pytest.mark.parametrize("k,m", [g for g in GEOMETRIES if g[0] <= 32])
def test_both_modes_are_one_function_up_to_k32(O, k, m):
    for r in MR.parity_reads():
        if len(r) >= k:
            got = MR.enumerate_read(r, k, m, full=True)
            assert (got.kmers, got.cuts, got.rets) == as_enumerated(O.enumerate(r, k, m)), (k, m, r)


@pytest.mark.parametrize("k,m", [(33, 21), (47, 21), (63, 21)])
def test_full_mode_gives_every_canonical_kmer_one_identity(k, m):
    reads = MR.tie_free_reads(k, m)
    assert MR.windows_tie_free(reads, k, m) and MR.windows_tie_free([MR.revcomp(r) for r in reads], k, m)
    identity = {}  # canonical k-mer -> the one identity it has, across all reads and both strands
    for r in reads:
        for strand in (r, MR.revcomp(r)):
            for can, ident in zip(MR.canonical_kmers(strand, k), MR.enumerate_read(strand, k, m, full=True).by_pos):
                assert identity.setdefault(can, ident) == ident, (k, m, can)
    distinct = {c for r in reads for c in MR.canonical_kmers(r, k)}
    full = MR.index_of(reads, k, m, full=True)
    assert len(full) == len(distinct) == len(identity)
    assert sum(full.values()) == sum(len(r) - k + 1 for r in reads)
    # the reason for the feature: the reference's truncated re-scan splits k-mers among several identities
    assert len(MR.index_of(reads, k, m, full=False)) > len(distinct)


def test_the_header_declares_the_field_and_the_enum(lib):
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    assert re.search(r"#define\s+BRISK_HIP_ABI_VERSION\s+4\b", hdr) and lib.brisk_hip_abi_version() == 4  # additions only
    assert re.search(r"\bBRISK_HIP_MINIMIZER_REFERENCE\s*=\s*0\b", hdr) and re.search(r"\bBRISK_HIP_MINIMIZER_FULL\s*=\s*1\b", hdr)
    # the field fills what was padding in both structs that carry it (count_mode stays their last member, no other member moves);
    # brisk_hip_layout has neither padding nor a struct_size: the handle's mode has a call of its own
    members = {}
    for name in ("brisk_hip_options", "brisk_hip_layout", "brisk_hip_snapshot_info"):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members[name] = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*[;,]", body)
    o, s = members["brisk_hip_options"], members["brisk_hip_snapshot_info"]
    assert o[o.index("minimizer_mode") - 1:o.index("minimizer_mode") + 2] == ["n_owners", "minimizer_mode", "arena_entries"] and o[-1] == "count_mode"
    assert s[s.index("minimizer_mode") - 1:s.index("minimizer_mode") + 2] == ["shift", "minimizer_mode", "n_entries"] and s[-1] == "count_mode"
    assert "minimizer_mode" not in members["brisk_hip_layout"]
    assert re.search(r"int\s+brisk_hip_get_minimizer_mode\(const brisk_hip_index \*h, uint32_t \*out\);", hdr)
    assert lib.brisk_hip_get_minimizer_mode(None, None) == 1  # EINVAL


def test_the_ctypes_structures_and_the_wrapper_follow():
    import inspect
    # in what was padding: every other member where it was before the field existed, the sizes unchanged
    O, S = hipapi._Options, hipapi._SnapshotInfo
    assert (O.minimizer_mode.size, O.minimizer_mode.offset, O.n_owners.offset, O.arena_entries.offset, O.count_mode.offset, C.sizeof(O)) == (4, 28, 24, 32, 56, 64)
    assert (S.minimizer_mode.size, S.minimizer_mode.offset, S.shift.offset, S.n_entries.offset, S.count_mode.offset, C.sizeof(S)) == (4, 52, 48, 56, 120, 128)
    assert "minimizer_mode" not in [n for n, _ in hipapi._Layout._fields_] and "brisk_hip_get_minimizer_mode" in hipapi.SYMBOLS
    assert hipapi.MINIMIZER_MODES == {"reference": 0, "full": 1} and brisk_amd.MINIMIZER_MODES is hipapi.MINIMIZER_MODES
    assert inspect.signature(brisk_amd.BriskHip.__init__).parameters["minimizer_mode"].default == "reference"
    with pytest.raises(ValueError):
        brisk_amd.BriskHip(63, 21, 14, minimizer_mode="whole")  # refused before any device call
    from brisk_amd import exchange
    assert inspect.signature(exchange.ShardedCounter.__init__).parameters["minimizer_mode"].default == "reference"


def snapshot_file(path, mode):
    raw = bytearray(pack_header(**FIELDS) + bytes(block_bytes(FIELDS["n_partitions"], FIELDS["n_entries"], FIELDS["key_words"])))
    raw[116] = mode
    with open(path, "wb") as f:
        f.write(raw)
    return str(path)


def test_the_header_reader_reports_byte_116(lib, tmp_path):
    full = snapshot_file(tmp_path / "full.snap", 1)
    old = snapshot_file(tmp_path / "old.snap", 0)
    assert brisk_amd.snapshot_info(full)["minimizer_mode"] == 1
    assert brisk_amd.snapshot_info(old)["minimizer_mode"] == 0  # every file written before the field existed
    assert {n: v for n, v in brisk_amd.snapshot_info(full).items() if n != "minimizer_mode"} == {n: v for n, v in brisk_amd.snapshot_info(old).items() if n != "minimizer_mode"}
    # a caller whose struct ends before the field: nothing is written past its size
    old_size = hipapi._SnapshotInfo.minimizer_mode.offset
    buf = (C.c_ubyte * C.sizeof(hipapi._SnapshotInfo))(*([0xAB] * C.sizeof(hipapi._SnapshotInfo)))
    info = hipapi._SnapshotInfo.from_buffer(buf)
    info.struct_size = old_size
    assert lib.brisk_hip_snapshot_info_read(full.encode(), C.byref(info)) == 0
    assert info.struct_size == old_size and info.k == 63 and info.shift == 4
    assert bytes(buf)[old_size:] == bytes([0xAB] * (C.sizeof(hipapi._SnapshotInfo) - old_size))
    with pytest.raises(brisk_amd.BriskHipError) as e:
        brisk_amd.snapshot_info(snapshot_file(tmp_path / "future.snap", 2))
    assert e.value.code == EFORMAT


def test_brisk_count_names_the_option_and_keeps_it_to_bulk():
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    src = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        brisk_amd.build_apps()
    run = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "--full-minimizers" in run.stdout and "minimizer_mode" in run.stdout
    fa = os.path.join(ROOT, "tests", "golden", "test.fa")
    for mode in ("--facade", "--mixed"):
        run = subprocess.run([exe, mode, fa, "63", "21", "14", "--full-minimizers"], capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "--bulk only" in run.stderr and "--full-minimizers" in run.stderr, mode
