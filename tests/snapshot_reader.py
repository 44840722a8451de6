"""A reader of index snapshot files in pure Python, written from DESIGN.md section 4.w ("File format, version 1") and not from the
library's C++: the tests parse saved files with it, so the document and the writer are checked against each other.

read(path) -> (header dict, list of blocks); a block is a dict with `partitions` and `counts` (uint32 arrays, one element per
non-empty partition), `keys` (uint64, shape (n_entries, key_words)), `data` (uint8: the count of every entry) and `bytes`."""
import struct

import numpy as np

MAGIC = b"BRSKSNP1"
HEADER_BYTES = 256
FIELDS_U32 = ("version", "header_bytes", "k", "m", "b", "data_bytes", "part_bits", "ext_bits", "cls_bits", "cls_width", "key_words", "shift")


def pack_header(**f):
    """the 256 header bytes from the documented layout (for tests that build files of their own)"""
    body = MAGIC + struct.pack("<12I", *(f[n] for n in FIELDS_U32))
    body += struct.pack("<3Q", f["n_entries"], f["n_partitions"], f["nb_skmers"]) + struct.pack("<3Q", *f["checksum"]) + struct.pack("<Q", f["n_blocks"])
    assert len(body) == 112
    return body + bytes(HEADER_BYTES - len(body))


def parse_header(raw):
    assert len(raw) >= HEADER_BYTES and raw[:8] == MAGIC, "not a snapshot"
    h = dict(zip(FIELDS_U32, struct.unpack_from("<12I", raw, 8)))
    h["n_entries"], h["n_partitions"], h["nb_skmers"] = struct.unpack_from("<3Q", raw, 56)
    h["checksum"] = struct.unpack_from("<3Q", raw, 80)
    (h["n_blocks"],) = struct.unpack_from("<Q", raw, 104)
    assert raw[112:HEADER_BYTES] == bytes(HEADER_BYTES - 112), "header padding is not zero"
    assert h["version"] == 1 and h["header_bytes"] == HEADER_BYTES
    return h


def block_bytes(n_pairs, n_entries, key_words):
    return 16 + 8 * n_pairs + 8 * key_words * n_entries + (n_entries + 7) // 8 * 8


def read(path):
    raw = open(path, "rb").read()
    h = parse_header(raw)
    kw = h["key_words"]
    at = HEADER_BYTES
    blocks = []
    for _ in range(h["n_blocks"]):
        assert at % 8 == 0
        n_pairs, reserved, n_ent = struct.unpack_from("<IIQ", raw, at)
        assert reserved == 0
        size = block_bytes(n_pairs, n_ent, kw)
        assert at + size <= len(raw), "the file ends inside a block"
        pairs = np.frombuffer(raw, "<u4", 2 * n_pairs, at + 16).reshape(-1, 2)
        keys = np.frombuffer(raw, "<u8", kw * n_ent, at + 16 + 8 * n_pairs).reshape(-1, kw)
        data_at = at + 16 + 8 * n_pairs + 8 * kw * n_ent
        data = np.frombuffer(raw, np.uint8, n_ent, data_at)
        assert raw[data_at + n_ent:at + size] == bytes(at + size - data_at - n_ent), "block padding is not zero"
        blocks.append(dict(partitions=pairs[:, 0].copy(), counts=pairs[:, 1].copy(), keys=keys, data=data, bytes=size, offset=at))
        at += size
    assert at == len(raw), "bytes after the last block"
    return h, blocks
