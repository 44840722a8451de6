"""The per-call (entry-id) protocol replayed on the oracle: the inputs of tests/test_percall_edges.py,
tests/test_percall_edges_cpu.py and tests/percall_worker.py and what the device must answer to them, call by call.  Nothing here
touches the device or the library under test.

The protocol is apps/counter.cpp's: every sequence goes through the enumerator, every vector (the k-mers of one super-k-mer, at most
k - m + 1 of them) through one upsert; an entry's identity is (k-mer, minimizer_idx), unhashed; a new entry takes the next dense id
and DATA 1 on the host, a found one (DATA + 1) % 256.  The last section replays k_upsert's slice allocation and the host's arena
growth without virtual memory management, which makes the arena sizes and the vectors that are resumed part-way predictable."""
import random
from collections import namedtuple

import numpy as np

import geometry_edges as G
import oracle

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
ABSENT = 0xffffffff

Vector = namedtuple("Vector", "seq lo hi idx ids newly")  # seq: index of the sequence; ids / newly: what upsert_kmers must return


def _rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def sequences(r):
    """One row's input, seeded from (k, m, b): 60 reads of 150 nt from a 900-nt genome, both strands; eight of them a second time,
    further on (vectors of found k-mers only, and, where a read starts inside a super-k-mer of another, found and new mixed); the
    low-complexity reads; one random sequence of 700 nt; one shorter than any k and an empty one."""
    rng = random.Random(r.k * 10000 + r.m * 100 + r.b)
    genome = _rnd(rng, 900)
    reads = []
    for _ in range(60):
        p = rng.randrange(0, len(genome) - 150 + 1)
        s = genome[p:p + 150]
        reads.append(s if rng.random() < 0.5 else "".join(COMP[c] for c in reversed(s)))
    reads = reads[:40] + reads[3:11] + reads[40:]
    return reads + ["A" * 150, "AC" * 75, "ACGTTGCA" * 20, _rnd(rng, 700), "ACG", ""]


def growth_sequences(r):
    """the arena-growth input of one row: random sequences of 5000 nt, GROWTH_NT[r] in all, and the first one again at the end (found
    k-mers, in partitions that have moved)"""
    rng = random.Random(r.k * 10000 + r.m * 100 + r.b + 7)
    seqs = [_rnd(rng, 5000) for _ in range(GROWTH_NT[r] // 5000)]
    return seqs + seqs[:1]


class Replay:
    """What the oracle says about the per-call protocol over `seqs`; computed once, shared, and left unchanged.
    streams[i]: O.enumerate(seqs[i])[:5] -- returned minimizer values, vector lengths, lo, hi, minimizer_idx;
    vectors: every vector in call order, with the (ids, newly) its upsert must return;
    entries: the identities (lo, hi, idx) in order of first appearance -- entries[id]; data[id]: the host's DATA at the end."""

    def __init__(self, O, k, m, seqs):
        self.k, self.m, self.seqs = k, m, list(seqs)
        self.streams, self.vectors, self.entries, self.data = [], [], [], []
        id_of = {}
        for si, s in enumerate(self.seqs):
            st = O.enumerate(s, k, m)[:5] if len(s) >= k else (np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64),
                                                               np.zeros(0, np.uint64), np.zeros(0, np.uint8))
            self.streams.append(st)
            p = 0
            for n in st[1].tolist():
                lo, hi, idx = (a[p:p + n] for a in st[2:5])
                ids, newly = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
                for j, ident in enumerate(zip(lo.tolist(), hi.tolist(), idx.tolist())):
                    e = id_of.get(ident)
                    if e is None:
                        e = id_of[ident] = len(self.entries)
                        self.entries.append(ident)
                        self.data.append(1)
                        newly[j] = 1
                    else:
                        self.data[e] = (self.data[e] + 1) % 256
                    ids[j] = e
                self.vectors.append(Vector(si, lo, hi, idx, ids, newly))
                p += n
            assert p == len(st[2])
        self.id_of = id_of

    def arrays(self, n=None):
        """(lo, hi, idx) of entries[:n] as the arrays find_kmers takes"""
        e = self.entries[:n]
        return (np.array([x[0] for x in e], np.uint64), np.array([x[1] for x in e], np.uint64), np.array([x[2] for x in e], np.uint8))

    def lines(self, n=None, data=None):
        """the dump of the first n entries as oracle.multiset_lines gives it"""
        lo, hi, idx = self.arrays(n)
        return oracle.multiset_lines(lo, hi, idx, (self.data if data is None else data)[:len(lo)], self.k)

    def figures(self):
        """the non-vacuity figures of tests/test_percall_edges_cpu.py"""
        n_new = sum(int(v.newly.sum()) for v in self.vectors)
        n_all = sum(len(v.ids) for v in self.vectors)
        return dict(entries=len(self.entries), vectors=len(self.vectors), longest=max(len(v.ids) for v in self.vectors), kmers=n_all, new=n_new,
                    found=n_all - n_new, mixed=sum(0 < int(v.newly.sum()) < len(v.newly) for v in self.vectors))


_replays = {}


def replay(O, r):
    """the replay of sequences(r), once per process"""
    if r not in _replays:
        _replays[r] = Replay(O, r.k, r.m, sequences(r))
    return _replays[r]


def oracle_count(O, r, seqs):
    """(lines, nb_kmers, nb_buckets): O.count of the sequences that hold a k-mer"""
    return O.count([s for s in seqs if len(s) >= r.k], r.k, r.m, r.b)


def partitions(O, r, rp, n=None):
    """partition of entries[:n] at a row without a routing-id extension: the oracle's bucket id without its low `shift` bits"""
    L = G.row_layout(r)
    assert L["ext_bits"] == 0, "with an extension the partition does not follow from the bucket id"
    h = O.index_new(r.k, r.m, r.b)
    try:
        return (O.bucket_ids(h, *rp.arrays(n)) >> np.uint32(L["shift"])).tolist()
    finally:
        O.index_free(h)


def flipped(rp, O, r, n=500):
    """[(lo, hi, idx, expected ids)] of the first n entries with one bit of the k-mer flipped -- the last nucleotide, and one of the
    first (as test_geometry_edges.test_index picks them): the id where the oracle's index of the same sequences has the k-mer under
    that minimizer_idx, 0xffffffff where it says absent"""
    flat, offs = oracle.pack_reads([s for s in rp.seqs if len(s) >= r.k])
    h = O.index_new(r.k, r.m, r.b)
    out = []
    try:
        O.index_insert_reads(h, flat, offs)
        lo, hi, idx = rp.arrays(n)
        for flip in (np.uint64(1), np.uint64(1) << np.uint64(2 * min(r.k, 32) - 1)):
            lo2 = lo ^ flip
            want = np.full(len(lo2), ABSENT, np.uint32)
            for j, ident in enumerate(zip(lo2.tolist(), hi.tolist(), idx.tolist())):
                present = O.index_get(h, *ident) >= 0
                assert present == (ident in rp.id_of)
                if present:
                    want[j] = rp.id_of[ident]
            out.append((lo2, hi, idx, want))
    finally:
        O.index_free(h)
    return out


# ---- k_upsert's allocation and the host's arena growth, replayed ------------------------------------------------------------------
FIRST_ARENA = 1 << 16  # entries of the arena brisk_hip_upsert_kmers asks for on an empty handle


def grow_cap(n):
    """brisk_insert.hip: the slots of a slice made for n entries"""
    return n + n // 4 + 8


def predict_cursor(entry_partitions):
    """The arena cursor after k_upsert has put entries into the partitions `entry_partitions` (one per entry, in insertion order):
    a partition that is full (cnt == cap, at first 0 == 0) moves to a new slice of grow_cap(cnt + 1) slots taken from the cursor;
    abandoned slices are not reused."""
    cnt, cap, cursor = {}, {}, 0
    for p in entry_partitions:
        c = cnt.get(p, 0)
        if c == cap.get(p, 0):
            cap[p] = grow_cap(c + 1)
            cursor += cap[p]
        cnt[p] = c + 1
    return cursor


Growth = namedtuple("Growth", "vector done n used arena")  # vector: index in Replay.vectors; done of n k-mers were in; arena: the new size


def predict_growths(rp, entry_partitions, limit=0):
    """The copy growths (no virtual memory management) of the per-call fill of a replay, as brisk_hip_upsert_kmers and ensure_arena
    make them: the arena starts at FIRST_ARENA entries; k_upsert stops at the first k-mer whose new slice would end beyond it; the
    host then asks for as many entries again as the arena has -- the new size is max(cap + cap / 4, used + cap) -- and goes on with
    the rest of the vector.  Returns ([Growth], cursor at the end); with limit (BRISK_ARENA_LIMIT), the list ends with the growth that
    is refused (used + cap > limit), its `arena` None."""
    cnt, cap, cursor, arena = {}, {}, 0, FIRST_ARENA
    out = []
    for vi, v in enumerate(rp.vectors):
        for j, (e, new) in enumerate(zip(v.ids.tolist(), v.newly.tolist())):
            if not new:
                continue
            p = entry_partitions[e]
            c = cnt.get(p, 0)
            if c == cap.get(p, 0):
                want = grow_cap(c + 1)
                while cursor + want > arena:
                    if limit and cursor + arena > limit:
                        out.append(Growth(vi, j, len(v.ids), cursor, None))
                        return out, cursor
                    arena = max(arena + arena // 4, cursor + arena)
                    out.append(Growth(vi, j, len(v.ids), cursor, arena))
                cap[p] = want
                cursor += want
            cnt[p] = c + 1
    return out, cursor


# The rows where the partition follows from the oracle's bucket id alone, and how much random sequence fills them: at (44, 23, 12) a
# partition is a bucket (2^24 of them: nearly every vector opens one, of 9, then 20, then 34 slots), at (31, 11, 4, pb 2) there are
# four (a slice move copies thousands of entries, every upsert walks thousands).
GROWTH_ROWS = [G.TABLE[13], G.TABLE[6]]
GROWTH_NT = {G.TABLE[13]: 60_000, G.TABLE[6]: 40_000}
_growth = {}


def growth_case(O, r):
    """(replay of growth_sequences(r), partition of every entry, predicted growths, predicted cursor), once per process"""
    if r not in _growth:
        rp = Replay(O, r.k, r.m, growth_sequences(r))
        parts = partitions(O, r, rp)
        _growth[r] = (rp, parts) + predict_growths(rp, parts)
    return _growth[r]


def arena_limit(growths):
    """a BRISK_ARENA_LIMIT between what the first growth asks for (used + arena entries: granted) and what the second does (refused)"""
    first, second = growths[0].used + FIRST_ARENA, growths[1].used + growths[0].arena
    assert first < second
    return (first + second) // 2
