"""numpy statement of brisk_hip_extract_packed, for the extraction tests (no device, no library): the packed stream's layout -- 16
nucleotides per uint32, the first one in the top bits, codes A0 C1 T2 G3 -- and the kept intervals of a stream gathered, nucleotide
by nucleotide, into a new one.  test_extract_cpu.py checks it against plain Python string slicing and the library's host packer; the
GPU tests then trust it."""
import numpy as np

SHIFTS = (30 - 2 * np.arange(16)).astype(np.uint32)
LETTERS = np.frombuffer(b"ACTG", np.uint8)


def pack_codes(codes, extra_words=0):
    """2-bit codes -> packed words, the last one zero padded, `extra_words` zero words after it"""
    v = np.asarray(codes, np.uint8)
    v = np.concatenate([v, np.zeros((-len(v)) % 16, np.uint8)]).reshape(-1, 16).astype(np.uint32)
    words = (v << SHIFTS).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([words, np.zeros(extra_words, np.uint32)])


def unpack_codes(words, n):
    """the first n nucleotides of a packed stream as 2-bit codes"""
    w = np.asarray(words, np.uint32)[:(n + 15) // 16]
    return ((w[:, None] >> SHIFTS) & 3).astype(np.uint8).reshape(-1)[:n]


def pack_reads(seqs, extra_words=2):
    """strings -> (packed words with `extra_words` zero words after the last, starts uint64[n + 1])"""
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    starts = np.zeros(len(bs) + 1, np.uint64)
    if bs:
        starts[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    flat = np.frombuffer(b"".join(bs), np.uint8)
    return pack_codes((flat >> 1) & 3, extra_words), starts


def extract_reference(words, starts, intervals):
    """-> (out_words with the two zero words after the last, out_starts uint64[n_out + 1], out_index uint64[n_out], n_out, n_nts)"""
    starts = np.asarray(starts, np.uint64).astype(np.int64)
    start = np.asarray(intervals["start"]).astype(np.int64)
    length = np.asarray(intervals["len"]).astype(np.int64)
    n_reads = len(starts) - 1
    assert len(start) == n_reads and (start + length <= starts[1:] - starts[:-1]).all()
    codes = unpack_codes(words, int(starts[-1]) if n_reads else 0)
    index = np.nonzero(length > 0)[0]
    lens = length[index]
    out_starts = np.zeros(len(index) + 1, np.uint64)
    out_starts[1:] = np.cumsum(lens, dtype=np.uint64)
    total = int(out_starts[-1])
    first = np.cumsum(lens) - lens
    src = np.repeat(starts[index] + start[index], lens) + (np.arange(total, dtype=np.int64) - np.repeat(first, lens))
    return pack_codes(codes[src], 2), out_starts, index.astype(np.uint64), len(index), total


def ascii_of(codes):
    return LETTERS[np.asarray(codes, np.uint8)].tobytes().decode()
