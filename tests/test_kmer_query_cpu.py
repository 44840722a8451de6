"""CPU-side checks of the per-k-mer get (brisk_hip_get_kmers): both entry points are declared, exported and bound, and the
slot layout helper the callers size their output with agrees with a plain statement of the layout."""
import os
import re

import numpy as np
import pytest

import brisk_amd
from brisk_amd import hipapi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brisk_hip_get_kmers", "brisk_hip_get_kmers_packed")


@pytest.fixture(scope="module")
def lib():
    brisk_amd.build_library()
    return hipapi.load()


def test_get_kmers_is_declared_exported_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared, s
        assert s in hipapi.SYMBOLS, s
        assert hasattr(lib, s), s
    assert lib.brisk_hip_abi_version() == 4  # additions only
    assert "uint16_t *out, uint64_t cap" in hdr and "uint16_t *d_out" in hdr


def _slots_by_hand(lens, k):
    base = [0]
    for n in lens:
        base.append(base[-1] + (n - k + 1 if n >= k else 0))
    return np.array(base, dtype=np.uint64)


@pytest.mark.parametrize("k", [1, 15, 31, 63])
def test_slot_layout_helper(k):
    rng = np.random.default_rng(k)
    lens = [0, k - 1, k, k + 1, 150, 0, 1, 2 * k] + [int(x) for x in rng.integers(0, 3 * k, 200)]
    lens = [n for n in lens if n >= 0]
    offs = np.zeros(len(lens) + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    got = hipapi.kmer_slots(offs, k)
    assert got.dtype == np.uint64 and len(got) == len(lens) + 1
    assert np.array_equal(got, _slots_by_hand(lens, k))
    # slot base[r] + i is the k-mer at nucleotide i of read r: every slot belongs to exactly one (read, position)
    owner = np.repeat(np.arange(len(lens)), np.diff(got).astype(np.int64))
    assert len(owner) == int(got[-1])
    assert brisk_amd.kmer_slots is hipapi.kmer_slots


def test_slot_layout_helper_edge_cases():
    assert np.array_equal(hipapi.kmer_slots(np.zeros(1, np.uint64), 31), np.zeros(1, np.uint64))  # no reads
    assert np.array_equal(hipapi.kmer_slots([0, 0, 0], 31), np.zeros(3, np.uint64))  # empty reads
    assert np.array_equal(hipapi.kmer_slots([0, 30, 61, 92], 31), np.array([0, 0, 1, 2], np.uint64))  # shorter than, equal to k
    # more slots than 32 bits count (50 M reads of 150 bp at k = 63 are 4.4 G)
    offs = np.array([0, 3 << 30, 6 << 30, 6 << 30], np.uint64)
    assert int(hipapi.kmer_slots(offs, 63)[-1]) == 2 * ((3 << 30) - 62)
