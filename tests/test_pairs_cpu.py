"""CPU: the paired-end additions at the C-ABI boundary (header, SYMBOLS, struct sizes) and the four numpy definitions the GPU tests
compare with -- intervals_from_fragments, pair_intervals, split_pairs, compose_intervals -- each against plain Python."""
import ctypes as C
import itertools
import os
import random
import re

import numpy as np
import pytest

import brisk_amd as B
from brisk_amd import hipapi
from intake_reference import invalid_run, valid_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IV = B.READ_INTERVAL_DTYPE
NEW = ["brisk_hip_fragment_intervals", "brisk_hip_pair_intervals", "brisk_hip_compose_intervals", "brisk_hip_extract_pairs_packed", "brisk_hip_trim_pairs_packed",
       "brisk_hip_trim_pairs_reads", "brisk_hip_clean_pairs_ascii", "brisk_hip_clean_pairs_reads"]


def iv(rows):
    return np.array(rows, np.uint32).reshape(-1, 2).copy().view(IV).reshape(-1)


def test_header_symbols_and_abi():
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in hipapi.SYMBOLS, s
        assert re.fullmatch(r"brisk_hip_[a-z_]+", s)
    assert sorted(declared) == sorted(hipapi.SYMBOLS)
    assert re.search(r"#define\s+BRISK_HIP_ABI_VERSION\s+4\b", hdr)
    top = hdr[:hdr.index("#ifndef")] if "#ifndef" in hdr[:200] else hdr[:hdr.index("typedef")]
    assert "brisk_hip_extract_pairs_packed" in top and "extract-paired-reads" in top and "Trimmomatic" in top  # the reference-counterpart block
    assert re.search(r"BRISK_HIP_PAIR_EACH\s*=\s*0,\s*BRISK_HIP_PAIR_ALL\s*=\s*1,\s*BRISK_HIP_PAIR_ANY\s*=\s*2", hdr)
    B.build_library()
    lib = hipapi.load()
    for s in NEW:
        assert hasattr(lib, s), s
    assert lib.brisk_hip_abi_version() == 4


def test_struct_sizes():
    assert C.sizeof(hipapi._PairCounts) == 64 == 8 * len(B.PAIR_COUNTS_FIELDS)
    assert B.PAIR_COUNTS_FIELDS == ("n_pairs_in", "n_pairs_kept", "n_single_first", "n_single_second", "n_pairs_dropped", "n_nts_pairs", "n_nts_singles", "reserved")
    assert C.sizeof(hipapi._Fragment) == B.FRAGMENT_DTYPE.itemsize == 16
    assert C.sizeof(C.c_uint32 * 2) == IV.itemsize == 8
    assert C.sizeof(hipapi._IntakeStats) == 8 * len(B.INTAKE_STATS_FIELDS)
    assert B.PAIR_MODES == {"each": 0, "all": 1, "any": 2}


def loop_intervals(frags, n_reads):
    out = [(0, 0)] * n_reads
    for f in frags:
        r, s, n = int(f["read"]), int(f["start"]), int(f["len"])
        if n > out[r][1]:  # strictly longer: of equal lengths the first one stays
            out[r] = (s, n)
    return out


def test_intervals_from_fragments():
    rng = random.Random(11)
    k = 9
    reads = []
    for i in range(300):
        kind = i % 6
        if kind == 0:
            reads.append(b"")
        elif kind == 1:
            reads.append(invalid_run(rng, rng.randint(1, 30)))
        elif kind == 2:
            reads.append(valid_run(rng, rng.randint(k, 60)))
        elif kind == 3:  # ties: equal-length fragments, the first wins
            n = rng.randint(k, 20)
            reads.append(valid_run(rng, n) + b"N" + valid_run(rng, n) + b"NN" + valid_run(rng, n))
        else:
            reads.append(b"N".join(valid_run(rng, rng.randint(1, 40)) for _ in range(rng.randint(2, 8))))
    frags, st = B.fragments_from_reads(reads, None, k)
    got = B.intervals_from_fragments(frags, len(reads))
    want = loop_intervals(frags, len(reads))
    assert [tuple(r) for r in got.tolist()] == want
    counts = np.bincount(frags["read"].astype(np.int64), minlength=len(reads))
    assert (counts == 0).any() and (counts == 1).any() and (counts > 2).any()
    ties = [r for r in range(len(reads)) if counts[r] >= 2 and sorted(frags["len"][frags["read"] == r])[-1] == sorted(frags["len"][frags["read"] == r])[-2]]
    assert len(ties) >= 20
    for r in ties:  # the first of the longest
        mine = frags[frags["read"] == r]
        assert got[r]["start"] == mine["start"][np.argmax(mine["len"])]
    for r in range(len(reads)):
        s, n = int(got[r]["start"]), int(got[r]["len"])
        assert all(c in b"ACGTacgt" for c in reads[r][s:s + n]) and (n == 0 or n >= k)
    assert len(B.intervals_from_fragments(frags[:0], 5)) == 5 and not B.intervals_from_fragments(frags[:0], 5)["len"].any()
    assert len(B.intervals_from_fragments(frags[:0], 0)) == 0
    with pytest.raises(ValueError):
        B.intervals_from_fragments(frags, int(frags["read"].max()))
    swapped = frags.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    with pytest.raises(ValueError) as e:
        B.intervals_from_fragments(swapped, len(reads))
    assert "row 11 " in str(e.value)


def test_pair_intervals_truth_table():
    """{kept, dropped}^2 for each x {whole kept, whole dropped}^2 for whole, in the three modes"""
    E = {True: (3, 20), False: (7, 0)}   # a dropped row may carry a start
    W = {True: (0, 50), False: (0, 0)}
    for ka, kb, wa, wb in itertools.product((True, False), repeat=4):
        each, whole = iv([E[ka], E[kb]]), iv([W[wa], W[wb]])
        assert B.pair_intervals(each, whole, "each").tolist() == each.tolist()
        assert B.pair_intervals(each, None, "each").tolist() == each.tolist()
        want_all = each.tolist() if ka and kb else [(0, 0), (0, 0)]
        assert B.pair_intervals(each, None, "all").tolist() == want_all
        want_any = [W[wa] if wa else (0, 0), W[wb] if wb else (0, 0)] if ka or kb else [(0, 0), (0, 0)]
        assert B.pair_intervals(each, whole, "any").tolist() == want_any
        assert B.pair_intervals(each, whole, 2).tolist() == want_any
    with pytest.raises(ValueError):
        B.pair_intervals(iv([(0, 1)] * 3), None, "each")
    with pytest.raises(ValueError):
        B.pair_intervals(iv([(0, 1)] * 2), None, "any")
    with pytest.raises(ValueError):
        B.pair_intervals(iv([(0, 1)] * 2), None, "some")
    with pytest.raises(ValueError):
        B.pair_intervals(iv([(0, 1)] * 2), None, 3)
    assert len(B.pair_intervals(iv([]), None, "all")) == 0


def test_split_pairs():
    rng = np.random.default_rng(5)
    v = np.zeros(2000, IV)
    v["start"] = rng.integers(0, 50, 2000)
    v["len"] = np.where(rng.random(2000) < 0.6, rng.integers(1, 200, 2000), 0)
    p, s, c = B.split_pairs(v)
    kp, ks, kv = p["len"] > 0, s["len"] > 0, v["len"] > 0
    assert not (kp & ks).any()                                    # disjoint
    assert np.array_equal(kp | ks, kv)                            # their union is the input's kept rows
    assert np.array_equal(p[kp], v[kp]) and np.array_equal(s[ks], v[ks])
    assert not p[~kp]["start"].any() and not s[~ks]["start"].any()
    assert np.array_equal(kp[0::2], kp[1::2])                     # pairs stay pairs
    assert not (ks[0::2] & ks[1::2]).any()                        # a single has no mate
    assert c["n_pairs_in"] == 1000 == c["n_pairs_kept"] + c["n_single_first"] + c["n_single_second"] + c["n_pairs_dropped"]
    assert min(c["n_pairs_kept"], c["n_single_first"], c["n_single_second"], c["n_pairs_dropped"]) >= 20
    assert c["n_pairs_kept"] * 2 == kp.sum() and c["n_single_first"] == ks[0::2].sum() and c["n_single_second"] == ks[1::2].sum()
    assert c["n_nts_pairs"] == int(v["len"][kp].sum()) and c["n_nts_singles"] == int(v["len"][ks].sum()) and c["reserved"] == 0
    assert set(c) == set(B.PAIR_COUNTS_FIELDS)
    with pytest.raises(ValueError):
        B.split_pairs(v[:3])
    p0, s0, c0 = B.split_pairs(v[:0])
    assert len(p0) == len(s0) == 0 and not any(c0.values())


def test_compose_intervals():
    rng = random.Random(3)
    n = 400
    outer = iv([(rng.randint(0, 30), rng.choice((0, 0, rng.randint(1, 100)))) for _ in range(n)])
    index = [r for r in range(n) if outer[r]["len"]]
    inner = []
    for r in index:
        L = int(outer[r]["len"])
        if rng.random() < 0.3:
            inner.append((rng.randint(0, L), 0))       # dropped by the second cut
        else:
            a = rng.randint(0, L - 1)
            inner.append((a, rng.randint(1, L - a)))
    inner = iv(inner)
    got = B.compose_intervals(outer, inner, index)
    want = [(0, 0)] * n
    for j, r in enumerate(index):
        if inner[j]["len"]:
            want[r] = (int(outer[r]["start"]) + int(inner[j]["start"]), int(inner[j]["len"]))
    assert [tuple(x) for x in got.tolist()] == want
    assert sum(1 for w in want if w[1]) >= 20 and sum(1 for j in range(len(index)) if not inner[j]["len"]) >= 20
    # the whole inner interval: the outer one again
    whole = iv([(0, int(outer[r]["len"])) for r in index])
    assert np.array_equal(B.compose_intervals(outer, whole, index)["len"], outer["len"])
    assert len(B.compose_intervals(outer, inner[:0], [])) == n and not B.compose_intervals(outer, inner[:0], [])["len"].any()
    bad = inner.copy()
    j = next(j for j in range(len(index)) if inner[j]["len"])
    bad[j]["len"] = outer[index[j]]["len"] - bad[j]["start"] + 1
    with pytest.raises(ValueError) as e:
        B.compose_intervals(outer, bad, index)
    assert "row %d" % j in str(e.value)
    with pytest.raises(ValueError):
        B.compose_intervals(outer, inner[:1], [n])
    with pytest.raises(ValueError):
        B.compose_intervals(outer, inner[:2], [index[1], index[0]])
