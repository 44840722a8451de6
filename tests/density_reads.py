"""A deterministic, error-bearing read generator for the dense-batch tests (numpy only; no Python list of a million strings).

`dense_reads` samples reads from a random genome on both strands and returns them as the flat buffers the C-ABI and the
oracle take: (flat uint8 ASCII, offs uint64[n + 1]).  What a sequencing run does to reads and the reference's harness does
to a FASTA record is applied on the way:

* a length mix (100 / 150 / 250) and a ragged tail of lengths k-2 .. k+2;
* per-base substitutions at rate `e`;
* with probability `p_n` per read a run of 1-10 `N`, after which the read is cut exactly as `oracle.fasta_sequences` cuts a
  record (counter.cpp:130-190): the pieces become sequences of their own, pieces shorter than k stay in the batch, empty ones
  do not exist;
* a family of repeats: one element of `repeat_len` bp planted at `repeat_copies` loci, every second copy with 2 % of its
  bases substituted, so that the partitions of its minimizers lie an order of magnitude above the mean;
* `n_special` homopolymer / short-tandem reads, and a share of lower-case reads (kept lower-case: the kernels and the oracle
  take the case-blind code (c >> 1) & 3).

With `cut=False` the reads are returned before the cut, `N` runs in place: tests write those out as FASTA text and compare
what `oracle.fasta_sequences` makes of it with the cut output (tests/test_density_cpu.py)."""
from __future__ import annotations

from typing import Tuple

import numpy as np

_LETTERS = np.frombuffer(b"ACTG", np.uint8)  # code -> letter (A0 C1 T2 G3; Kmers.cpp:442-444); complement = code ^ 2
_N = ord("N")
_CHUNK = 1 << 17  # reads per numpy pass


def random_genome(length: int, seed: int) -> np.ndarray:
    return np.random.default_rng([seed, 0x6e0]).integers(0, 4, length, dtype=np.uint8)


def _offsets(lens: np.ndarray) -> np.ndarray:
    offs = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, dtype=np.uint64, out=offs[1:])
    return offs


def _special_reads(rng, n: int) -> list:
    """homopolymers, short tandem repeats, and reads that run into a poly-A tail (codes)"""
    units = [[0], [2], [1], [3], [0, 1], [0, 1, 3], [0, 1, 3, 2], [0, 1, 3, 2, 2, 3, 1, 0], [0, 0, 0, 2], [1, 3]]
    out = []
    for i in range(n):
        u = np.array(units[i % len(units)], np.uint8)
        L = (100, 150, 250)[(i // len(units)) % 3]
        r = np.tile(u, L // len(u) + 1)[:L].copy()
        if i % 7 == 3:  # a random head, then the tandem
            h = int(rng.integers(20, 80))
            r[:h] = rng.integers(0, 4, h, dtype=np.uint8)
        out.append(r)
    return out


def dense_reads(n_reads: int, k: int, genome_len: int, seed: int, e: float = 0.01, p_n: float = 0.002, repeat_len: int = 0,
                repeat_copies: int = 0, n_special: int = 300, lower_share: float = 0.02, ragged_share: float = 0.02,
                cut: bool = True, genome: np.ndarray | None = None) -> Tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng([seed, n_reads, k])
    g = random_genome(genome_len, seed) if genome is None else genome
    assert len(g) == genome_len and genome_len > 600
    if repeat_len and repeat_copies:
        g = g.copy()
        assert 200 <= repeat_len <= 2000 and repeat_copies * repeat_len * 2 < genome_len
        element = rng.integers(0, 4, repeat_len, dtype=np.uint8)
        # non-overlapping loci: one per stretch of genome_len / copies
        stride = genome_len // repeat_copies
        for c in range(repeat_copies):
            at = c * stride + int(rng.integers(0, stride - repeat_len))
            copy = element.copy()
            if c & 1:
                hit = rng.random(repeat_len) < 0.02
                copy[hit] = (copy[hit] + rng.integers(1, 4, int(hit.sum()), dtype=np.uint8)) & 3
            g[at:at + repeat_len] = copy
    n_special = min(n_special, n_reads // 2)
    n_sampled = n_reads - n_special
    # lengths
    lens = rng.choice(np.array([100, 150, 250], np.int64), n_sampled, p=[0.25, 0.5, 0.25])
    ragged = rng.random(n_sampled) < ragged_share
    lens[ragged] = rng.integers(max(k - 2, 1), k + 3, int(ragged.sum()))
    special = _special_reads(rng, n_special)
    it = np.int32 if genome_len < (1 << 31) - 1024 else np.int64
    parts = []  # (flat, lens) per chunk of whole reads, cut chunk by chunk: no array of the batch's size besides the output
    for c0 in range(0, n_sampled, _CHUNK):
        c1 = min(c0 + _CHUNK, n_sampled)
        ln = lens[c0:c1].astype(it)
        tot = int(ln.sum())
        start = (rng.random(c1 - c0) * (genome_len - ln + 1)).astype(it)
        rev = rng.random(c1 - c0) < 0.5
        first = (np.cumsum(ln, dtype=np.int64) - ln).astype(it)
        within = np.arange(tot, dtype=it) - np.repeat(first, ln)
        rrev = np.repeat(rev, ln)
        pos = np.repeat(start, ln) + np.where(rrev, np.repeat(ln - 1, ln) - within, within)
        codes = g[pos] ^ (rrev.view(np.uint8) << 1)
        if e > 0:
            hit = rng.integers(0, tot, int(rng.binomial(tot, e)))  # (a base drawn twice is substituted once)
            codes[hit] = (codes[hit] + rng.integers(1, 4, len(hit), dtype=np.uint8)) & 3
        letters = _LETTERS[codes]
        if lower_share > 0:
            low = np.repeat(rng.random(c1 - c0) < lower_share, ln)
            letters[low] |= 0x20
        if p_n > 0:
            for r in np.nonzero(rng.random(c1 - c0) < p_n)[0]:
                run = int(rng.integers(1, 11))
                at = int(rng.integers(0, ln[r]))
                letters[first[r] + at: first[r] + min(at + run, ln[r])] = _N
        parts.append((letters, ln.astype(np.int64)))
    if special:
        parts.append((_LETTERS[np.concatenate(special)], np.array([len(s) for s in special], np.int64)))
    if cut:
        parts = [(lambda f, o: (f, (o[1:] - o[:-1]).astype(np.int64)))(*cut_at_invalid(f, _offsets(ln))) for f, ln in parts]
    flat = np.ascontiguousarray(np.concatenate([p[0] for p in parts])) if parts else np.zeros(0, np.uint8)
    return flat, _offsets(np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.int64))


def cut_at_invalid(flat: np.ndarray, offs: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """What the harness makes of records (counter.cpp:130-190): a sequence ends at the first character outside [ACGTacgt], the
    next one starts at the next valid character; nothing empty is kept."""
    valid = np.zeros(256, bool)
    valid[np.frombuffer(b"ACGTacgt", np.uint8)] = True
    keep = valid[flat]
    is_start = keep.copy()
    is_start[1:] &= ~keep[:-1]  # a valid character after an invalid one ...
    read_start = np.zeros(len(flat) + 1, bool)
    read_start[offs[:-1].astype(np.int64)] = True
    is_start |= keep & read_start[:-1]  # ... or the first character of a read
    new_pos = np.cumsum(keep, dtype=np.int64) - 1  # index of every kept character in the output
    starts = new_pos[is_start]
    out = flat[keep]
    new_offs = np.empty(len(starts) + 1, np.uint64)
    new_offs[:-1] = starts
    new_offs[-1] = len(out)
    return np.ascontiguousarray(out), new_offs


def take_reads(flat: np.ndarray, offs: np.ndarray, which: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The reads `which` (indices, any order, repeats allowed) as buffers of their own."""
    which = np.asarray(which, np.int64)
    o = offs.astype(np.int64)
    ln = o[which + 1] - o[which]
    new_offs = _offsets(ln)
    tot = int(new_offs[-1])
    first = np.cumsum(ln) - ln
    src = np.repeat(o[which], ln) + (np.arange(tot, dtype=np.int64) - np.repeat(first, ln))
    return np.ascontiguousarray(flat[src]), new_offs


def substitute(flat: np.ndarray, rate: float, seed: int) -> np.ndarray:
    """Fresh substitutions at `rate` per base (case kept)."""
    rng = np.random.default_rng([seed, 0x5b5])
    out = flat.copy()
    hit = np.nonzero(rng.random(len(flat)) < rate)[0]
    code = (out[hit] >> 1) & 3
    out[hit] = _LETTERS[(code + rng.integers(1, 4, len(hit), dtype=np.uint8)) & 3] | (out[hit] & 0x20)
    return out


def concat_reads(parts) -> Tuple[np.ndarray, np.ndarray]:
    flats = [p[0] for p in parts]
    lens = np.concatenate([(p[1][1:] - p[1][:-1]).astype(np.int64) for p in parts])
    return np.ascontiguousarray(np.concatenate(flats)), _offsets(lens)


def as_strings(flat: np.ndarray, offs: np.ndarray) -> list:
    b = flat.tobytes()
    o = offs.astype(np.int64)
    return [b[o[i]:o[i + 1]].decode() for i in range(len(o) - 1)]


def poly_a_reads(n: int, k: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """Reads that meet the query's `minimizer == 0` stop (counter.cpp:304-306): a random head, a run of A of at least k, a
    random tail; and plain poly-A."""
    rng = np.random.default_rng([seed, 0xa11a])
    reads = []
    for i in range(n):
        head = _LETTERS[rng.integers(0, 4, int(rng.integers(0, 90)), dtype=np.uint8)]
        tail = _LETTERS[rng.integers(0, 4, int(rng.integers(0, 90)), dtype=np.uint8)]
        run = np.full(int(rng.integers(k, k + 60)), ord("A"), np.uint8)
        reads.append(run if i % 5 == 0 else np.concatenate([head, run, tail]))
    return np.ascontiguousarray(np.concatenate(reads)), _offsets(np.array([len(r) for r in reads], np.int64))


def entry_diff(got, want, k: int, limit: int = 10) -> str:
    """Where two indexes differ: got / want are (lo, hi, idx, cnt) arrays of unhashed entries.  Returns the first `limit`
    entries missing from got, extra in got, and present in both with another count, as `KMER idx count` lines (sorted by
    (hi, lo, idx)); '' when the entry sets are equal."""
    dt = np.dtype([("hi", np.uint64), ("lo", np.uint64), ("idx", np.uint8)])

    def keyed(e):
        key = np.empty(len(e[0]), dt)
        key["hi"], key["lo"], key["idx"] = e[1], e[0], e[2]
        order = np.argsort(key, order=("hi", "lo", "idx"), kind="stable")
        return key[order], np.asarray(e[3])[order]

    gk, gc = keyed(got)
    wk, wc = keyed(want)
    missing = ~np.isin(wk, gk)
    extra = ~np.isin(gk, wk)
    both_w = wk[~missing]
    both_g = gk[~extra]
    assert len(both_w) == len(both_g) or len(np.unique(gk)) != len(gk) or len(np.unique(wk)) != len(wk)
    lines = []

    def kmer(key):
        v = (int(key["hi"]) << 64) | int(key["lo"])
        return "".join("ACTG"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))

    def section(title, keys, counts, other=None):
        if len(keys) == 0:
            return
        lines.append(f"{title}: {len(keys)}")
        for i in range(min(limit, len(keys))):
            lines.append(f"  {kmer(keys[i])} {int(keys[i]['idx'])} {int(counts[i])}" + (f" (want {int(other[i])})" if other is not None else ""))

    section("missing from the index under test", wk[missing], wc[missing])
    section("extra in the index under test", gk[extra], gc[extra])
    if len(both_w) == len(both_g):
        cg, cw = gc[~extra], wc[~missing]
        bad = cg != cw
        section("present with another count", both_g[bad], cg[bad], cw[bad])
    else:
        lines.append(f"duplicate entries: {len(gk) - len(np.unique(gk))} in the index under test, {len(wk) - len(np.unique(wk))} in the expectation")
    return "\n".join(lines)
