"""CPU-side checks of saturating counts (brisk_hip_options.count_mode): the boundary only -- the header declares the field and the
enum, the library and the ctypes structures agree with it, the snapshot header reader reports byte 112, brisk_count names the
option.  No device is needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import brisk_amd
from brisk_amd import hipapi
from snapshot_reader import HEADER_BYTES, block_bytes, pack_header

FIELDS = dict(version=1, header_bytes=256, k=63, m=21, b=14, data_bytes=1, part_bits=24, ext_bits=0, cls_bits=0, cls_width=1, key_words=2, shift=4,
              n_entries=5, n_partitions=2, nb_skmers=77, checksum=(5, 9, 0x0123456789ABCDEF), n_blocks=1)
EFORMAT = 8


@pytest.fixture(scope="module")
def lib():
    brisk_amd.build_library()
    return hipapi.load()


def header():
    return open(os.path.join(ROOT, "include", "brisk_hip.h")).read()


def struct_fields(name):
    """the member names of `typedef struct NAME { ... } NAME;` in the header, in order, comments stripped"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split(None, 1)[1] if not decl.startswith("void") else decl[len("void"):]
        out += [re.sub(r"[\s*]|\[.*\]", "", n) for n in names.split(",")]
    return out


def snapshot_file(path, count_mode):
    raw = bytearray(pack_header(**FIELDS) + bytes(block_bytes(FIELDS["n_partitions"], FIELDS["n_entries"], FIELDS["key_words"])))
    raw[112] = count_mode
    with open(path, "wb") as f:
        f.write(raw)
    return str(path)


def test_the_header_declares_the_field_the_enum_and_abi_4(lib):
    hdr = header()
    assert re.search(r"#define\s+BRISK_HIP_ABI_VERSION\s+4\b", hdr) and lib.brisk_hip_abi_version() == 4  # additions only
    assert re.search(r"\bBRISK_HIP_COUNTS_WRAP\s*=\s*0\b", hdr) and re.search(r"\bBRISK_HIP_COUNTS_SATURATE\s*=\s*1\b", hdr)
    assert struct_fields("brisk_hip_options")[-1] == "count_mode"  # at the end: the struct grows through struct_size
    assert struct_fields("brisk_hip_layout")[-1] == "count_mode"
    assert struct_fields("brisk_hip_snapshot_info")[-1] == "count_mode"
    assert re.search(r"uint32_t\s+count_mode;", hdr)


def test_the_library_exports_what_the_header_declares(lib):
    declared = sorted(set(re.findall(r"\b(brisk_hip_[a-z_]+)\s*\(", header())))
    assert declared == sorted(hipapi.SYMBOLS)
    for s in declared:
        assert hasattr(lib, s), s


def test_the_ctypes_structures_follow_the_header():
    assert [n for n, _ in hipapi._Options._fields_] == struct_fields("brisk_hip_options")
    assert [n for n, _ in hipapi._Layout._fields_] == struct_fields("brisk_hip_layout")
    want = struct_fields("brisk_hip_snapshot_info")
    assert [n for n, _ in hipapi._SnapshotInfo._fields_] == want
    assert hipapi._Options.count_mode.size == 4 and hipapi._Options.count_mode.offset == hipapi._Options.immediate_inserts.offset + 4
    assert hipapi.COUNT_MODES == {"wrap": 0, "saturate": 1} and brisk_amd.COUNT_MODES is hipapi.COUNT_MODES


def test_the_wrapper_takes_and_documents_the_mode():
    import inspect
    sig = inspect.signature(brisk_amd.BriskHip.__init__)
    assert sig.parameters["count_mode"].default == "wrap"
    with pytest.raises(ValueError):
        brisk_amd.BriskHip(63, 21, 14, count_mode="clamp")  # refused before any device call
    for meth in ("merge", "intersect", "count_spectrum", "prune", "read_profile"):
        assert "255" in getattr(brisk_amd.BriskHip, meth).__doc__ and "saturat" in getattr(brisk_amd.BriskHip, meth).__doc__, meth
    from brisk_amd import exchange
    assert "count_mode" in inspect.signature(exchange.ShardedCounter.__init__).parameters


def test_the_header_reader_reports_byte_112(lib, tmp_path):
    sat = snapshot_file(tmp_path / "sat.snap", 1)
    old = snapshot_file(tmp_path / "old.snap", 0)
    assert brisk_amd.snapshot_info(sat)["count_mode"] == 1
    assert brisk_amd.snapshot_info(old)["count_mode"] == 0
    assert {n: v for n, v in brisk_amd.snapshot_info(sat).items() if n != "count_mode"} == {n: v for n, v in brisk_amd.snapshot_info(old).items() if n != "count_mode"}
    # a caller with the struct as it was before the field: nothing is written past its size
    old_size = hipapi._SnapshotInfo.count_mode.offset
    assert old_size == 120
    buf = (C.c_ubyte * C.sizeof(hipapi._SnapshotInfo))(*([0xAB] * C.sizeof(hipapi._SnapshotInfo)))
    info = hipapi._SnapshotInfo.from_buffer(buf)
    info.struct_size = old_size
    assert lib.brisk_hip_snapshot_info_read(sat.encode(), C.byref(info)) == 0
    assert info.struct_size == old_size and info.k == 63 and info.file_bytes == os.path.getsize(sat)
    assert bytes(buf)[old_size:] == bytes([0xAB] * (C.sizeof(hipapi._SnapshotInfo) - old_size))
    # a mode this library does not know is not a snapshot it can read
    with pytest.raises(brisk_amd.BriskHipError) as e:
        brisk_amd.snapshot_info(snapshot_file(tmp_path / "future.snap", 2))
    assert e.value.code == EFORMAT


def test_brisk_count_help_names_the_option():
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe):
        brisk_amd.build_apps()
    run = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "--saturate" in run.stdout and "255" in run.stdout
    # outside --bulk it is refused like the other device options, before any device call
    fa = os.path.join(ROOT, "tests", "golden", "test.fa")
    run = subprocess.run([exe, "--facade", fa, "31", "11", "4", "--saturate"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "--bulk only" in run.stderr
