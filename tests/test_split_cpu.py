"""CPU: read splitting at the C-ABI boundary (header, SYMBOLS, struct size, exported symbols) and its numpy definition,
fragments_from_slots, against a plain Python loop over crafted slot arrays; the two counter identities and the link to the
solid_run rule on every case; the gather reference against string slicing; and the read generator of the GPU tests."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import brisk_amd as B
from brisk_amd import hipapi
from density_reads import dense_reads
from extract_reference import ascii_of, pack_reads, unpack_codes
from split_reference import as_table, fragment_case, gather_reference, host_slots_model, loop_fragments, slot_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["brisk_hip_solid_runs", "brisk_hip_extract_fragments_packed", "brisk_hip_split_packed", "brisk_hip_split_reads"]
K = 9
SOLID_MINS = (0, 1, 2, 255, 256)
MIN_LENS = (0, K, K + 1, K + 7)


def test_header_symbols_struct_and_exports():
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in hipapi.SYMBOLS, s
    assert sorted(declared) == sorted(hipapi.SYMBOLS)
    assert re.search(r"#define\s+BRISK_HIP_ABI_VERSION\s+4\b", hdr)
    top = hdr[:hdr.index("#ifndef")]
    assert all(s in top for s in NEW)  # the reference-counterpart block
    body = re.search(r"typedef struct brisk_hip_split_stats \{(.*?)\} brisk_hip_split_stats;", hdr, re.S).group(1)
    assert tuple(re.findall(r"uint64_t\s+(\w+);", body)) == B.SPLIT_STATS_FIELDS
    assert B.SPLIT_STATS_FIELDS == ("n_reads", "n_reads_kept", "n_fragments", "n_slots", "n_solid", "n_short", "n_nts_in", "n_nts_out")
    assert C.sizeof(hipapi._SplitStats) == 64 == 8 * len(B.SPLIT_STATS_FIELDS)
    assert "can hold MORE nucleotides than the input" in hdr  # the room rule of the other extract calls does not hold here
    B.build_library()
    lib = hipapi.load()
    for s in NEW:
        assert hasattr(lib, s), s
    assert lib.brisk_hip_abi_version() == 4


@pytest.fixture(scope="module")
def cases():
    return slot_cases(random.Random(2626), K, n_random=600, big=False)


def solid_run_intervals(counts, found, base, k, solid_min):
    return B.intervals_from_profile(B.profile_from_slots(counts, found, base, solid_min), k, B.select_rule("solid_run"))


def test_fragments_from_slots_against_a_plain_loop(cases):
    counts, found, base, n_nts = cases
    sizes = set((base[1:] - base[:-1]).tolist())
    assert {0, 1, 2, 63, 64, 65, 4095, 4096, 4097} <= sizes
    assert (found & (counts == 0)).any()  # a present slot whose count wrapped to 0
    ends_solid = [r for r in range(len(base) - 2) if base[r + 1] > base[r] and base[r + 2] > base[r + 1] and found[int(base[r + 1]) - 1] and found[int(base[r + 1])]
                  and counts[int(base[r + 1]) - 1] >= 2 and counts[int(base[r + 1])] >= 2]
    assert len(ends_solid) >= 5  # a solid last slot next to a solid first slot
    seen = set()
    for solid_min in SOLID_MINS:
        link = solid_run_intervals(counts, found, base, K, solid_min)
        for min_len in MIN_LENS:
            got, st = B.fragments_from_slots(counts, found, base, K, solid_min, min_len, n_nts_in=n_nts)
            want, want_st = loop_fragments(counts, found, base, K, solid_min, min_len, n_nts)
            assert [tuple(int(x) for x in row) for row in got.tolist()] == want, (solid_min, min_len)
            assert st == want_st, (solid_min, min_len)
            # the two identities
            assert st["n_solid"] == (st["n_nts_out"] - st["n_fragments"] * (K - 1)) + st["n_short"]
            assert st["n_nts_out"] == int(got["len"].astype(np.int64).sum())
            # ordered by read, then by start; inside the read; at least L long
            key = got["read"].astype(np.int64) * (1 << 32) + got["start"]
            assert (np.diff(key) > 0).all()
            slots = (base[1:] - base[:-1]).astype(np.int64)[got["read"].astype(np.int64)]
            assert (got["start"].astype(np.int64) + got["len"] <= slots + K - 1).all() and (got["len"] >= max(min_len, K)).all()
            if min_len <= K:  # the first longest fragment of a read is the solid_run rule's interval; no fragment where that is empty
                first_longest = {}
                for r, s, n in want:
                    if n > first_longest.get(r, (0, 0))[1]:
                        first_longest[r] = (s, n)
                for r in range(len(base) - 1):
                    assert (int(link[r]["start"]), int(link[r]["len"])) == first_longest.get(r, (0, 0)), (solid_min, r)
            seen.add((solid_min, min_len, st["n_fragments"] > 0, st["n_short"] > 0))
    assert (256, 0, False, False) in seen and (0, 0, True, False) in seen and (2, K + 7, True, True) in seen
    st0 = B.fragments_from_slots(counts, found, base, K, 0, 0)[1]
    assert st0["n_solid"] == int(found.sum()) > B.fragments_from_slots(counts, found, base, K, 1, 0)[1]["n_solid"]
    none = B.fragments_from_slots(counts[:0], found[:0], base[:1], K)
    assert len(none[0]) == 0 and none[0].dtype == B.FRAGMENT_DTYPE and not any(none[1].values())
    # without n_nts_in a read without a slot counts as empty
    assert B.fragments_from_slots(counts, found, base, K)[1]["n_nts_in"] == sum(int(n) + K - 1 for n in (base[1:] - base[:-1]) if n)


def test_the_big_read_of_the_gpu_cases():
    counts, found, base, n_nts = slot_cases(random.Random(1), K, n_random=0)
    assert int(base[1]) == 3 * 4096 + 5
    rows, _ = loop_fragments(counts[:int(base[1])], found[:int(base[1])], base[:2], K, 2, 0, 0)
    assert [s + n - (K - 1) - 1 for _, s, n in rows] == [63, 128, 193, 4095, 8192, 12289, 3 * 4096 + 4]  # the last solid slot of every run
    got, st = B.fragments_from_slots(counts, found, base, K, 2, 0, n_nts_in=n_nts)
    assert [tuple(int(x) for x in row) for row in got[:len(rows)].tolist()] == rows and st["n_nts_in"] == n_nts


def test_gather_reference_is_string_slicing():
    rng = random.Random(77)
    reads, rows = fragment_case(rng)
    table = as_table(rows)
    assert {(s % 16, n % 16) for _, s, n in rows} == {(a, b) for a in range(16) for b in range(16)}
    assert {1, 2, 3} <= {n for _, _, n in rows}
    per_read = np.bincount(table["read"].astype(np.int64), minlength=len(reads))
    assert (per_read == 0).any() and (per_read >= 3).any() and per_read[0] == 0 and per_read[-1] == 0
    assert any(a == b for a, b in zip(rows, rows[1:]))                                                      # the same row twice in a row
    assert any(a[0] == b[0] and b[1] < a[1] + a[2] for a, b in zip(rows, rows[1:]))                         # overlapping rows
    assert sorted(rows, key=lambda r: r[0]) == rows
    words, starts = pack_reads(reads)
    out, out_starts, total = gather_reference(words, starts, table)
    want = "".join(reads[r][s:s + n] for r, s, n in rows)
    assert total == len(want) and ascii_of(unpack_codes(out, total)) == want
    assert len(out) == (total + 15) // 16 + 2 and not out[-2:].any()
    assert out_starts.tolist() == np.concatenate(([0], np.cumsum([n for _, _, n in rows]))).tolist()
    whole = as_table([(r, 0, len(s)) for r, s in enumerate(reads)] * 2)
    assert gather_reference(words, starts, whole)[2] == 2 * int(starts[-1])                                  # more out than in
    empty = gather_reference(words, starts, table[:0])
    assert empty[2] == 0 and empty[0].tolist() == [0, 0] and empty[1].tolist() == [0]
    with pytest.raises(AssertionError):
        gather_reference(words, starts, as_table([(0, 0, len(reads[0]) + 1)]))


@pytest.mark.parametrize("k", (63, 31))
def test_the_error_reads_split(k):
    """what the composed GPU tests assert of error_reads(k), told here from a model of the index (k-mer hashing): with the first two
    thirds of the reads indexed, some read has two fragments, some has none, some runs are short, and there are more fragments than kept reads"""
    flat, offs = dense_reads(3000, k, 24_000, 7, e=0.01, n_special=40)  # extract_worker.error_reads(k)
    n = len(offs) - 1
    counts, found, base = host_slots_model(flat, offs, k, 2 * n // 3)
    assert int(base[-1]) == int(np.maximum((offs[1:] - offs[:-1]).astype(np.int64) - (k - 1), 0).sum())
    for solid_min, min_len in ((2, 0), (2, k + 20), (1, 0)):
        frags, st = B.fragments_from_slots(counts, found, base, k, solid_min, min_len, n_nts_in=int(offs[-1]))
        per_read = np.bincount(frags["read"].astype(np.int64), minlength=n)
        assert (per_read >= 2).sum() >= 20 and (per_read == 0).sum() >= 20, (solid_min, min_len)
        assert st["n_fragments"] > st["n_reads_kept"] > 0
        assert st["n_short"] > 0 or min_len == 0
    assert B.fragments_from_slots(counts, found, base, k, 2, k + 20)[1]["n_short"] > 0
    assert B.fragments_from_slots(counts, found, base, k, 256, 0)[1]["n_fragments"] == 0
