"""CPU-side checks of the de Bruijn adjacency calls (brisk_hip_adjacency / _degree_spectrum / _prune_degrees): the host definitions in
brisk_amd/hipapi.py -- the yardstick of tests/test_graph.py -- against loops written out nucleotide by nucleotide and slot by slot,
the sum identity, graph_figures on hand-made matrices, and the boundary: header, SYMBOLS, brisk_count's usage text.  No device."""
import os
import random
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from brisk_amd import hipapi

NEW = ["brisk_hip_adjacency", "brisk_hip_degree_spectrum", "brisk_hip_prune_degrees", "brisk_hip_graph_phase_ms"]


def packed(s):
    """kmer_s of a string as enumerate() returns it: leftmost nucleotide in the highest bits, codes of "ACTG\""""
    v = 0
    for ch in s:
        v = (v << 2) | "ACTG".index(ch)
    return v & ((1 << 64) - 1), v >> 64


@pytest.mark.parametrize("k", (31, 32, 33, 63))
def test_neighbour_strings_against_a_loop(k):
    rng = random.Random(k)
    xs = ["".join(rng.choice("ACGT") for _ in range(k)) for _ in range(40)] + ["A" * k, "G" * k, "AC" * (k // 2) + "A" * (k % 2)]
    lo, hi = zip(*(packed(x) for x in xs))
    got = hipapi.neighbour_strings(np.array(lo, np.uint64), np.array(hi, np.uint64), k)
    want = []
    for x in xs:
        for c in "ACTG":
            s = ""
            for i in range(1, k):
                s += x[i]
            want.append((s + c).encode())
        for c in "ACTG":
            s = c
            for i in range(k - 1):
                s += x[i]
            want.append(s.encode())
    assert len(got) == 8 * len(xs) and all(len(g) == k for g in got)
    assert [bytes(g) for g in got] == want
    assert hipapi.neighbour_strings(np.zeros(0, np.uint64), np.zeros(0, np.uint64), k) == []


def random_slots(seed, n):
    rng = np.random.default_rng(seed)
    found = rng.random(8 * n) < 0.4
    counts = np.where(found, rng.choice([0, 0, 1, 1, 2, 3, 254, 255], 8 * n), 0).astype(np.uint8)  # present entries with count 0 among them
    assert (found & (counts == 0)).any()
    return counts, found


@pytest.mark.parametrize("min_count", (0, 1, 2, 255, 256))
def test_adjacency_from_slots_against_a_loop(min_count):
    counts, found = random_slots(5, 300)
    got = hipapi.adjacency_from_slots(counts, found, min_count)
    want = []
    for e in range(300):
        a = 0
        for j in range(8):
            if found[8 * e + j] and int(counts[8 * e + j]) >= min_count:
                a |= 1 << j
        want.append(a)
    assert got.dtype == np.uint8 and got.tolist() == want
    if min_count == 0:
        assert (got != 0).any() and np.array_equal(got, hipapi.adjacency_from_slots(np.zeros_like(counts), found, 0))  # presence alone
    with pytest.raises(ValueError):
        hipapi.adjacency_from_slots(counts[:-1], found[:-1], 0)


@pytest.mark.parametrize("min_count", (0, 1, 2, 255, 300))
def test_degree_spectrum_from_adjacency_against_a_loop_and_the_sum_identity(min_count):
    rng = np.random.default_rng(9)
    adj = rng.integers(0, 256, 2000).astype(np.uint8)
    own = rng.choice([0, 1, 1, 2, 7, 255], 2000).astype(np.uint8)
    got = hipapi.degree_spectrum_from_adjacency(adj, own, min_count)
    want = [0] * hipapi.DEGREE_CLASSES
    for a, c in zip(adj.tolist(), own.tolist()):
        if c < min_count:
            want[25] += 1
        else:
            want[hipapi.degree_class(bin(a >> 4).count("1"), bin(a & 15).count("1"))] += 1
    assert got.dtype == np.uint64 and got.shape == (26,) and got.tolist() == want
    assert int(got.sum()) == len(adj)
    assert int(hipapi.degree_spectrum_from_adjacency(adj[:0], own[:0], min_count).sum()) == 0


def test_degree_class_and_mask():
    assert hipapi.DEGREE_CLASSES == 26
    assert [hipapi.degree_class(l, r) for l in range(5) for r in range(5)] == list(range(25))
    for bad in ((5, 0), (0, 5), (-1, 0)):
        with pytest.raises(ValueError):
            hipapi.degree_class(*bad)
    assert hipapi.degree_mask([(0, 0), (0, 1), (1, 0)]) == 0b100011 and hipapi.degree_mask(0x21) == 0x21 and hipapi.degree_mask([]) == 0


def test_graph_figures_on_hand_made_matrices():
    s = np.zeros(26, np.uint64)
    f = hipapi.graph_figures(s)
    assert f == dict(nodes=0, edge_ends=0, isolated=0, dead_ends=0, simple=0, branching=0, below=0)
    s[hipapi.degree_class(1, 1)] = 100  # a path: 100 simple nodes and its two ends, one isolated node, 7 entries below the threshold
    s[hipapi.degree_class(0, 1)] = 1
    s[hipapi.degree_class(1, 0)] = 1
    s[hipapi.degree_class(0, 0)] = 1
    s[25] = 7
    f = hipapi.graph_figures(s)
    assert f == dict(nodes=103, edge_ends=202, isolated=1, dead_ends=2, simple=100, branching=0, below=7)
    s[hipapi.degree_class(1, 2)] = 3  # forks, a fork that is also a dead end on its other side, a node with everything
    s[hipapi.degree_class(0, 3)] = 2
    s[hipapi.degree_class(4, 4)] = 1
    f = hipapi.graph_figures(s)
    assert f == dict(nodes=109, edge_ends=202 + 9 + 6 + 8, isolated=1, dead_ends=4, simple=100, branching=6, below=7)
    # symmetric in left and right
    t = np.concatenate([s[:25].reshape(5, 5).T.reshape(25), s[25:]])
    assert hipapi.graph_figures(t) == f
    with pytest.raises(ValueError):
        hipapi.graph_figures(np.zeros(25))


def test_the_new_symbols_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    for s in NEW:
        assert re.search(r"\bint %s\(brisk_hip_index \*h" % s, header), s
        assert s in hipapi.SYMBOLS
    assert "sum to nb_kmers" in header and "FULL-MODE INDEX" in header.upper()
    usage = open(os.path.join(ROOT, "brisk_amd", "apps", "brisk_count.cpp")).read()
    assert "--degrees FILE" in usage and "--prune-degrees L:R" in usage
    for name in ("adjacency", "adjacency_device", "degree_spectrum", "prune_degrees"):
        assert callable(getattr(hipapi.BriskHip, name))
