"""CPU: spectral read correction at the C-ABI boundary (header, SYMBOLS, struct sizes, exported symbols) and its numpy definitions:
sites_from_slots against a plain Python loop over crafted slot arrays, with both counter identities on every case and every class
seen; corrections_from_candidates against a loop with 0, 1, 2 and 3 passing candidates; the window and patch references against
string slicing."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import brisk_amd as B
from brisk_amd import hipapi
from correct_reference import (STATS, as_corrections, as_sites, candidate_strings, code_of, loop_corrections, loop_sites, patch_reference, patch_strings, weak_cases, window_case,
                               windows_reference)
from extract_reference import ascii_of, pack_reads, unpack_codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["brisk_hip_weak_sites", "brisk_hip_candidate_windows", "brisk_hip_decide_sites", "brisk_hip_apply_corrections", "brisk_hip_correct_packed", "brisk_hip_correct_reads"]
K = 9
SOLID_MINS = (0, 1, 2, 255, 256)
MIN_COVERS = (1, K // 2, K)


def test_header_symbols_structs_and_exports():
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in hipapi.SYMBOLS, s
    assert sorted(declared) == sorted(hipapi.SYMBOLS)
    assert re.search(r"#define\s+BRISK_HIP_ABI_VERSION\s+4\b", hdr)
    top = hdr[:hdr.index("#ifndef")]
    assert all(s in top for s in NEW)  # the reference-counterpart block
    body = re.search(r"typedef struct brisk_hip_correct_stats \{(.*?)\} brisk_hip_correct_stats;", hdr, re.S).group(1)
    assert tuple(re.findall(r"uint64_t\s+(\w+);", body)) == B.CORRECT_STATS_FIELDS == STATS
    assert C.sizeof(hipapi._CorrectStats) == 88 == 8 * len(B.CORRECT_STATS_FIELDS)
    assert B.SITE_DTYPE.itemsize == 16 and B.CORRECTION_DTYPE.itemsize == 16
    assert re.search(r"typedef struct brisk_hip_site \{ uint64_t read; uint32_t pos, cover; \}", hdr)
    assert re.search(r"typedef struct brisk_hip_correction \{ uint64_t read; uint32_t pos; uint8_t from, to; uint16_t cover; \}", hdr)
    assert [B.CORRECTION_DTYPE.fields[n][1] for n in ("read", "pos", "from", "to", "cover")] == [0, 8, 12, 13, 14]
    for name in ("sites_from_slots", "corrections_from_candidates", "SITE_DTYPE", "CORRECTION_DTYPE", "CORRECT_STATS_FIELDS"):
        assert hasattr(B, name), name
    for name in ("weak_sites", "candidate_windows", "decide_sites", "apply_corrections", "correct_packed", "correct_reads"):
        assert callable(getattr(B.BriskHip, name)), name
    B.build_library()
    lib = hipapi.load()
    for s in NEW:
        assert hasattr(lib, s), s
    assert lib.brisk_hip_abi_version() == 4


@pytest.fixture(scope="module")
def cases():
    return weak_cases(random.Random(2727), K)


def test_sites_from_slots_against_a_plain_loop(cases):
    counts, found, base = cases
    sizes = set((base[1:] - base[:-1]).tolist())
    assert {0, 1, 2, K - 1, K, 63, 64, 65, 4095, 4096, 4097} <= sizes
    weak2 = ~(found & (counts >= 2))
    edges = [r for r in range(len(base) - 2) if base[r + 1] > base[r] and base[r + 2] > base[r + 1] and weak2[int(base[r + 1]) - 1] and weak2[int(base[r + 1])]]
    assert len(edges) >= 5  # a weak last slot next to a weak first slot
    assert (found & (counts == 0)).any()  # a present slot whose count wrapped to 0: solid only at solid_min 0
    seen = dict.fromkeys(("n_sites", "n_skip_whole", "n_skip_long", "n_skip_short"), 0)
    shapes = set()
    for solid_min in SOLID_MINS:
        for min_cover in MIN_COVERS:
            got, st = B.sites_from_slots(counts, found, base, K, solid_min, min_cover)
            want, want_st = loop_sites(counts, found, base, K, solid_min, min_cover)
            assert [tuple(int(x) for x in row) for row in got.tolist()] == want, (solid_min, min_cover)
            assert st == want_st, (solid_min, min_cover)
            # the two identities (the second with the decision counters at zero: nothing has been decided)
            assert st["n_runs"] == st["n_sites"] + st["n_skip_whole"] + st["n_skip_long"] + st["n_skip_short"]
            assert st["n_corrected"] == st["n_ambiguous"] == st["n_unresolved"] == 0 and st["n_sites"] == len(got)
            for key in seen:
                seen[key] += st[key]
            # ordered by read, then by pos; two sites of a read at least k + 1 apart; the window inside the read
            key = got["read"].astype(np.int64) * (1 << 32) + got["pos"]
            assert (np.diff(key) > 0).all()
            same = got["read"][1:] == got["read"][:-1]
            assert (np.diff(got["pos"].astype(np.int64))[same] >= K + 1).all()
            slots = (base[1:] - base[:-1]).astype(np.int64)[got["read"].astype(np.int64)]
            w = B.site_windows(got, K)
            assert (w["start"].astype(np.int64) + w["len"] <= slots + K - 1).all() and (got["cover"] >= min_cover).all() and (got["cover"] <= K).all()
            shapes |= {(int(c), "left" if s == 0 else "right" if s + n == ns + K - 1 else "inner") for c, s, n, ns in zip(got["cover"], w["start"], w["len"], slots)}
            if solid_min == 256:  # no slot is solid: every read with a slot is one whole run
                assert st["n_sites"] == 0 and st["n_skip_whole"] == st["n_runs"] == int((base[1:] > base[:-1]).sum()) and st["n_weak"] == st["n_slots"]
    assert all(v > 0 for v in seen.values()), seen
    assert {(K, "inner"), (K, "left"), (K, "right"), (K - 1, "left"), (K - 1, "right"), (1, "left"), (1, "right")} <= shapes
    assert not any(kind == "inner" and c != K for c, kind in shapes)
    assert B.sites_from_slots(counts, found, base, K, 2, None)[1] == B.sites_from_slots(counts, found, base, K, 2, 0)[1] == B.sites_from_slots(counts, found, base, K, 2, K)[1]
    with pytest.raises(ValueError):
        B.sites_from_slots(counts, found, base, K, 2, K + 1)
    empty, st = B.sites_from_slots(np.zeros(0, np.uint8), np.zeros(0, bool), np.zeros(1, np.uint64), K)
    assert len(empty) == 0 and empty.dtype == B.SITE_DTYPE and not any(st.values())


def test_corrections_from_candidates_against_a_loop():
    rng = random.Random(5)
    sites, cc, cf, frm = [], [], [], []
    n_pass_seen = set()
    for s in range(400):
        cover = rng.randint(1, K)
        sites.append((s // 3, (s % 3) * (2 * K + 2) + K, cover))
        frm.append(rng.randrange(4))
        n_pass = s % 4 if s < 40 else rng.choice((0, 1, 1, 2, 3))
        passing = rng.sample(range(3), n_pass)
        n_pass_seen.add(n_pass)
        for c in range(3):
            cnt = [rng.choice((2, 3, 200)) for _ in range(cover)]
            fnd = [True] * cover
            if c not in passing:
                x = rng.randrange(cover)
                if rng.random() < 0.5:
                    cnt[x] = 1
                else:
                    fnd[x], cnt[x] = False, 0
            cc += cnt
            cf += fnd
    assert n_pass_seen == {0, 1, 2, 3}
    t = as_sites(sites)
    cc, cf = np.array(cc, np.uint8), np.array(cf, bool)
    for solid_min in (0, 1, 2, 3, 256):
        got, cnt = B.corrections_from_candidates(cc, cf, t, solid_min, frm)
        want, (n_c, n_a, n_u) = loop_corrections(cc, cf, sites, solid_min, frm)
        assert [tuple(int(x) for x in row) for row in got.tolist()] == want, solid_min
        assert cnt == {"n_sites": len(sites), "n_corrected": n_c, "n_ambiguous": n_a, "n_unresolved": n_u}
        assert cnt["n_sites"] == cnt["n_corrected"] + cnt["n_ambiguous"] + cnt["n_unresolved"]
        assert (got["from"] != got["to"]).all() and (got["to"] < 4).all()
        if solid_min == 2:
            assert n_c > 0 and n_a > 0 and n_u > 0
        if solid_min == 256:
            assert n_u == len(sites)
    with pytest.raises(ValueError):
        B.corrections_from_candidates(cc[:-1], cf[:-1], t, 2, frm)
    got, cnt = B.corrections_from_candidates(np.zeros(0, np.uint8), np.zeros(0, bool), as_sites([]), 2)
    assert len(got) == 0 and got.dtype == B.CORRECTION_DTYPE and not any(cnt.values())


def test_window_and_patch_references_against_string_slicing():
    rng = random.Random(27)
    k = 31
    reads, rows = window_case(rng, k)
    sites = as_sites(rows)
    words, starts = pack_reads(reads)
    out, out_starts, n_nts = windows_reference(words, starts, sites, k)
    cands = candidate_strings(reads, sites, k)
    assert len(cands) == 3 * len(rows) and n_nts == sum(len(c) for c in cands)
    assert ascii_of(unpack_codes(out, n_nts)) == "".join(cands)
    assert out_starts.tolist() == np.concatenate(([0], np.cumsum([len(c) for c in cands]))).tolist()
    assert (out[-2:] == 0).all() and len(out) == (n_nts + 15) // 16 + 2
    for (r, pos, cover), trio in zip(rows, zip(cands[0::3], cands[1::3], cands[2::3])):
        a = max(0, pos - k + 1)
        assert sorted(c[pos - a] for c in trio) == sorted(set("ACGT") - {reads[r][pos]}) and [code_of(c[pos - a]) for c in trio] == sorted(code_of(c[pos - a]) for c in trio)
        assert all(len(c) == cover + k - 1 and c[:pos - a] + reads[r][pos] + c[pos - a + 1:] == reads[r][a:a + cover + k - 1] for c in trio)
    # every offset within a word: where a window starts, how long it is, where its substitution lies -- in the output and in the source
    w = B.site_windows(sites, k)
    assert np.array_equal(w["len"], sites["cover"] + k - 1)
    at = out_starts[:-1].astype(np.int64)
    sub = at + np.repeat(sites["pos"].astype(np.int64) - w["start"], 3)
    src = np.repeat(starts[sites["read"].astype(np.int64)].astype(np.int64) + sites["pos"], 3)
    full = set(range(16))
    assert set((at % 16).tolist()) == full and set((np.repeat(w["len"], 3) % 16).tolist()) == full and set((sub % 16).tolist()) == full and set((src % 16).tolist()) == full
    assert (sites["pos"] == 0).any() and any(pos == len(reads[r]) - 1 for r, pos, _ in rows) and 3 * len(rows) > 256
    # the patch: every row's letter, nothing else
    corr = []
    for r, s in enumerate(reads):
        for pos in sorted(rng.sample(range(len(s)), min(len(s), rng.choice((0, 1, 2, 5))))):
            f = code_of(s[pos])
            corr.append((r, pos, f, rng.choice([x for x in range(4) if x != f]), 1))
    table = as_corrections(corr)
    patched, per_read = patch_strings(reads, table)
    got = patch_reference(words, starts, table)
    assert np.array_equal(got, pack_reads(patched)[0]) and sum(per_read) == len(corr)
    assert sum(a != b for s, p in zip(reads, patched) for a, b in zip(s, p)) == len(corr)
    assert np.array_equal(patch_reference(words, starts, as_corrections([])), words)
