"""CPU-side checks of index snapshots (brisk_hip_save / brisk_hip_load / brisk_hip_snapshot_info_read): the boundary only --
header, symbol table, constants, wrapper signatures, refusals that return before any device is touched, the header reader
(which needs no device) against headers built here from the layout DESIGN.md section 4.w documents, and the app's options.
What the kernels move is tests/test_snapshot.py (GPU)."""
import ctypes as C
import inspect
import os
import re

import pytest

import brisk_amd
from brisk_amd import hipapi
from snapshot_reader import HEADER_BYTES, block_bytes, pack_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["brisk_hip_save", "brisk_hip_load", "brisk_hip_snapshot_info_read"]
EINVAL, EIO, EFORMAT = 1, 7, 8
FIELDS = dict(version=1, header_bytes=256, k=63, m=21, b=14, data_bytes=1, part_bits=24, ext_bits=0, cls_bits=0, cls_width=1, key_words=2, shift=4,
              n_entries=5, n_partitions=2, nb_skmers=77, checksum=(5, 9, 0x0123456789ABCDEF), n_blocks=1)


@pytest.fixture(scope="module")
def lib():
    brisk_amd.build_library()
    return hipapi.load()


def header():
    return open(os.path.join(ROOT, "include", "brisk_hip.h")).read()


def write_file(path, fields, body_bytes=None):
    """a header from `fields` and a body of zeros as long as the format says (or as long as the caller says)"""
    if body_bytes is None:
        body_bytes = block_bytes(fields["n_partitions"], fields["n_entries"], fields["key_words"]) if fields["n_blocks"] else 0
    with open(path, "wb") as f:
        f.write(pack_header(**fields) + bytes(body_bytes))
    return str(path)


def test_declared_listed_and_exported(lib):
    declared = set(re.findall(r"\b(brisk_hip_[a-z_]+)\s*\(", header()))
    for name in NAMES:
        assert name in declared, name
        assert name in hipapi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.brisk_hip_abi_version() == 4  # additions only
    assert re.search(r"#define\s+BRISK_HIP_ABI_VERSION\s+4\b", header())


def test_status_codes_and_flags():
    hdr = header()
    for name, value in (("EIO", 7), ("EFORMAT", 8), ("LOAD_COMPACT", 0), ("LOAD_ROOM", 1)):
        assert re.search(r"\bBRISK_HIP_%s\s*=\s*%d\b" % (name, value), hdr), name
    assert hipapi.STATUS[7] == "EIO" and hipapi.STATUS[8] == "EFORMAT"


def test_wrapper_signatures():
    H = brisk_amd.BriskHip
    assert list(inspect.signature(H.save).parameters) == ["self", "path"]
    sig = inspect.signature(H.load)
    assert list(sig.parameters) == ["self", "path", "room"] and sig.parameters["room"].default is False
    assert isinstance(inspect.getattr_static(H, "open"), classmethod)
    sig = inspect.signature(H.open)
    assert list(sig.parameters) == ["path", "device", "room", "kw"] and sig.parameters["device"].default == 0 and sig.parameters["room"].default is False
    assert sig.parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert "part_bits = 0 if ext_bits > 0 else part_bits" in H.open.__doc__
    assert list(inspect.signature(brisk_amd.snapshot_info).parameters) == ["path"]


def test_null_handle_or_path_is_einval_without_a_device(lib, tmp_path):
    n = C.c_uint64(7)
    info = hipapi._SnapshotInfo(C.sizeof(hipapi._SnapshotInfo))
    good = write_file(tmp_path / "good.snap", FIELDS).encode()
    assert lib.brisk_hip_save(None, good, C.byref(n)) == EINVAL
    assert lib.brisk_hip_save(None, None, None) == EINVAL
    assert lib.brisk_hip_load(None, good, 0, C.byref(n)) == EINVAL
    assert lib.brisk_hip_load(None, None, 1, None) == EINVAL
    assert lib.brisk_hip_snapshot_info_read(None, C.byref(info)) == EINVAL
    assert lib.brisk_hip_snapshot_info_read(good, None) == EINVAL
    assert n.value == 7  # nothing written


def test_a_header_built_from_the_document_is_read_back_field_for_field(tmp_path):
    path = write_file(tmp_path / "a.snap", FIELDS)
    got = brisk_amd.snapshot_info(path)
    for name, want in FIELDS.items():
        assert got[name] == want, name
    assert got["file_bytes"] == os.path.getsize(path) == HEADER_BYTES + block_bytes(2, 5, 2)
    # an empty index is a header and nothing else; one-word keys
    empty = dict(FIELDS, k=31, m=15, key_words=1, shift=0, part_bits=24, n_entries=0, n_partitions=0, n_blocks=0, nb_skmers=0, checksum=(0, 0, 0))
    got = brisk_amd.snapshot_info(write_file(tmp_path / "e.snap", empty))
    assert all(got[name] == want for name, want in empty.items()) and got["file_bytes"] == HEADER_BYTES
    assert brisk_amd.snapshot_info(tmp_path / "e.snap") == got  # a path object is a path


def test_what_is_not_a_snapshot_is_eformat(tmp_path):
    def code(path):
        with pytest.raises(brisk_amd.BriskHipError) as e:
            brisk_amd.snapshot_info(path)
        return e.value.code
    good = write_file(tmp_path / "good.snap", FIELDS)
    raw = open(good, "rb").read()
    wrong_magic = tmp_path / "magic.snap"
    wrong_magic.write_bytes(b"BRSKSNP2" + raw[8:])
    assert code(wrong_magic) == EFORMAT
    fasta = tmp_path / "reads.fa"
    fasta.write_bytes(b">r\n" + b"ACGT" * 100 + b"\n")
    assert code(fasta) == EFORMAT
    assert code(write_file(tmp_path / "future.snap", dict(FIELDS, version=2))) == EFORMAT
    # n_entries against the file's length: one entry more than the bytes hold, and bytes for entries the header does not have
    assert code(write_file(tmp_path / "more.snap", dict(FIELDS, n_entries=6, checksum=(6, 9, 1)), body_bytes=block_bytes(2, 5, 2))) == EFORMAT
    assert code(write_file(tmp_path / "less.snap", dict(FIELDS, n_entries=4, checksum=(4, 9, 1)), body_bytes=block_bytes(2, 5, 2) + 64)) == EFORMAT
    assert code(write_file(tmp_path / "huge.snap", dict(FIELDS, n_entries=1 << 60, checksum=(1 << 60, 9, 1)), body_bytes=block_bytes(2, 5, 2))) == EFORMAT


def test_a_missing_or_short_file_is_eio(tmp_path):
    for path in (tmp_path / "nothing.snap", tmp_path / "no_such_dir" / "x.snap"):
        with pytest.raises(brisk_amd.BriskHipError) as e:
            brisk_amd.snapshot_info(path)
        assert e.value.code == EIO
    short = tmp_path / "short.snap"
    short.write_bytes(pack_header(**FIELDS)[:100])
    with pytest.raises(brisk_amd.BriskHipError) as e:
        brisk_amd.snapshot_info(short)
    assert e.value.code == EIO


def test_brisk_count_knows_the_options():
    src = open(os.path.join(ROOT, "brisk_amd", "apps", "brisk_count.cpp")).read()
    for opt, call in (("--save", "brisk_hip_save"), ("--load", "brisk_hip_load")):
        assert '"%s"' % opt in src and call + "(" in src, opt
    assert "BRSKSNP1" in src and "brisk_hip_snapshot_info_read(" in src  # a set operation's FILE is recognised by its magic


def test_the_product_still_never_touches_the_oracle():
    from test_capi_cpu import test_product_never_touches_the_oracle
    test_product_never_touches_the_oracle()
    assert os.path.exists(os.path.join(ROOT, "brisk_amd", "csrc", "brisk_snapshot.hip"))  # and the walk saw the new file
