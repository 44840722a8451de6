"""The record builder of the k63 m21 scan bodies (anchored_record in brisk_scan.hip): a super-k-mer's window is loaded at a
position fixed by its minimizer, so what decides whether a record is right is the geometry of the super-k-mer -- how many k-mers,
where the minimizer lies, which strand -- and where its window falls in the packed stream.  Every test compares with the oracle's
records or index, bit for bit; what the reads must cover is established from the oracle's records alone, on the CPU, before
anything runs on the device."""
import os
import random

import numpy as np
import pytest

import oracle
from test_kmer_query import as_u16, assert_slots, expected_all, oracle_index, packed_on_device

pytestmark = pytest.mark.gpu

K, M = 63, 21
W = K - M
NTS = "ACTG"  # codes 0..3 (nuc2int, Kmers.cpp:442-444)
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def _genome_reads(rng, n, glen, lo=63, hi=170):
    genome = "".join(rng.choice("ACGT") for _ in range(glen))
    out = []
    for _ in range(n):
        L = rng.randint(lo, hi)
        p = rng.randrange(0, glen - L)
        s = genome[p:p + L]
        out.append(revcomp(s) if rng.random() < 0.5 else s)
    return out


def corner_reads(seed):
    """A few hundred reads of 63..170 nt from a short genome, homopolymers, short periods (tie rules, windows won by the all-A key)"""
    rng = random.Random(seed)
    reads = _genome_reads(rng, 320, 3000)
    reads += ["A" * 63, "A" * 170, "T" * 105, "C" * 64, "G" * 150, "AC" * 80, "ACG" * 50, "ACGT" * 40, "AAT" * 45, "ACGTTGCA" * 20,
              "A" * 70 + "ACGTTGCA" * 10, "T" * 104 + "A", "AAAAAAAAAAAAAAAAAAAAAC" * 7, "CAAAAAAAAAAAAAAAAAAAAA" * 7]
    g = "".join(rng.choice("ACGT") for _ in range(100))
    reads += ["A" * 50 + g, g + "A" * 60, "T" * 40 + g + "T" * 30]
    return reads


class Rec:
    """One oracle record, and what can be told from it alone: the nucleotides of its span (the compacted string with the bucket put
    back and the minimizer's hash inverted), hence the strand and the position of the span in its read."""

    def __init__(self, O, read, c, bucket, n, idx0p, b):
        sr = (M - b + 1) // 2
        self.words, self.bucket, self.n, self.idx0p = tuple(int(x) for x in c), int(bucket), int(n), int(idx0p)
        self.idx_first = self.idx0p - sr
        self.idx_end = self.idx_first + self.n - 1
        C = sum(w << (64 * i) for i, w in enumerate(self.words))
        cut = 2 * (self.idx_end + sr)
        S = ((C >> cut) << (cut + 2 * b)) | (self.bucket << cut) | (C & ((1 << cut) - 1))
        h = (S >> (2 * self.idx_end)) & ((1 << (2 * M)) - 1)
        S ^= (h ^ O.mix_inv(h, M)) << (2 * self.idx_end)
        self.L = K + self.n - 1
        assert S >> (2 * self.L) == 0
        s = "".join(NTS[(S >> (2 * (self.L - 1 - i))) & 3] for i in range(self.L))
        f, r = read.find(s), read.find(revcomp(s))
        assert f >= 0 or r >= 0, "a record whose nucleotides are not in its read"
        self.strand = None if (f >= 0 and r >= 0) else ("fwd" if f >= 0 else "rev")  # None: cannot be told
        self.pos = f if f >= 0 else r  # of the span's first nt in the read
        # nucleotides of the read before the minimizer's first, and the read index just past its last
        self.mini_from = self.pos + (self.idx_end if self.strand == "rev" else self.L - self.idx_end - M)
        self.mini_to = self.mini_from + M

    def key(self):
        return self.words + (self.bucket, self.n, self.idx0p)

    def last_nt(self, q0):
        """stream index of the nucleotide at bit 0 of the builder's window (af_last_nt in brisk_scan.hip), q0: of the read's first"""
        if self.strand == "rev":
            return q0 + self.pos + self.idx_end + (16 * 7 - 1 - W)
        return q0 + self.pos + self.L + (W - 1) - self.idx_end


def oracle_records(O, reads, b):
    h = O.index_new(K, M, b)
    out = []
    for s in reads:
        c, bucket, n, idx0 = O.records(h, s, K, M, b)
        out.append([Rec(O, s, c[i], bucket[i], n[i], idx0[i], b) for i in range(len(n))])
    O.index_free(h)
    return out


# The range of idx' of a record's first k-mer is [suff_reduc, suff_reduc + top]: minimizer_idx 0..top.  A reversed vector begins where
# its minimizer is about to leave: top = k - m = 42.  A forward one begins with a minimizer that has just entered (0) or that a
# re-scan has just found, and get_minimizer sees the low 64 bits of a k-mer only (Kmers.cpp:371): its windows 32..42 are all zero, a
# later one of them never beats the first strictly and the tie rules only lower the position, so top = 32 there -- no forward
# record of k = 63 has a first k-mer with its minimizer higher up.
TOP = {"fwd": 32, "rev": W}
CORNERS = [(what, strand) for what in ("n=1", "n=43", "idx_first=0", "idx_first=top") for strand in ("fwd", "rev")]


def corners_covered(recs):
    have = set()
    for r in (r for per_read in recs for r in per_read):
        if r.strand is None:
            continue
        assert r.idx_first <= TOP[r.strand]
        for what, hit in (("n=1", r.n == 1), ("n=43", r.n == W + 1), ("idx_first=0", r.idx_first == 0), ("idx_first=top", r.idx_first == TOP[r.strand])):
            if hit:
                have.add((what, r.strand))
    return have


def pack_stream(reads, fill):
    """The packed stream of the reads, exactly (nts + 15) // 16 + 2 words: 16 nts per word, the first in the top two bits; the unused
    bits of the last word and the two words behind it hold `fill`."""
    codes = np.concatenate([(np.frombuffer(r.encode(), np.uint8) >> 1) & 3 for r in reads]).astype(np.uint64)
    nts = len(codes)
    n_words = (nts + 15) // 16
    padded = np.concatenate([codes, np.full(n_words * 16 - nts, fill & 3, np.uint64)]).reshape(n_words, 16)
    words = np.zeros(n_words, np.uint64)
    for j in range(16):
        words |= padded[:, j] << np.uint64(30 - 2 * j)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return np.concatenate([words.astype(np.uint32), np.full(2, fill, np.uint32)]), offs


def scan_records(ix, d_packed_ptr, d_starts, n_reads, bound):
    import torch
    Wd = ix.record_words
    d_rec = torch.zeros(max(bound, 1) * Wd, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    n_rec = ix.scan_packed(d_packed_ptr, d_starts.data_ptr(), n_reads, d_rec.data_ptr(), bound)
    ix.sync()
    rec = d_rec.cpu().numpy().view(np.uint64)[: n_rec * Wd].reshape(n_rec, Wd)
    ext = ix.layout["ext_bits"]
    return sorted(tuple(int(x) for x in r[: Wd - 1]) + ((int(r[Wd - 1]) & 0xffffffff) >> ext, (int(r[Wd - 1]) >> 32) & 0xff, (int(r[Wd - 1]) >> 40) & 0xff)
                  for r in rec)


# the seeds were chosen on the CPU, from the oracle's records, so that the coverage asserted below holds
CORNER_SEED = {14: 1, 7: 1}


@pytest.mark.parametrize("b", [14, 7])
def test_geometry_corners(B, O, b):
    """n = 1 and n = k - m + 1, idx' of the first k-mer at both ends of its range, both strands of each: (63, 21, 14), and
    (63, 21, 7) for another suff_reduc and a four-word record"""
    import torch
    reads = corner_reads(CORNER_SEED[b])
    recs = oracle_records(O, reads, b)
    missing = [c for c in CORNERS if c not in corners_covered(recs)]
    assert not missing, missing
    want = sorted(r.key() for per_read in recs for r in per_read)
    with B.BriskHip(K, M, b) as ix:
        assert not ix.layout["cls_bits"]
        d_packed, d_starts, offs = packed_on_device(ix, reads)
        bound = ix.scan_bound(d_starts.data_ptr(), len(reads))
        got = scan_records(ix, d_packed.data_ptr(), d_starts, len(reads), bound)
    assert got == want


def _end_batches(O, b=14):
    """Batches of 1, 2 and 65 reads whose first read has a minimizer within its first 43 nts and whose last read's last super-k-mer
    is reversed / forward with one k-mer: the builder's window then reaches below the stream's first word and beyond its last."""
    rng = random.Random(77)
    pool = _genome_reads(rng, 2000, 3000)
    recs = oracle_records(O, pool, b)
    head = [i for i, rr in enumerate(recs) if rr and any(r.strand and r.mini_to <= 43 for r in rr)]
    last = lambda rr: max(rr, key=lambda r: r.pos + r.L)
    tail = {"rev": [i for i, rr in enumerate(recs) if rr and last(rr).strand == "rev"],
            "fwd1": [i for i, rr in enumerate(recs) if rr and last(rr).strand == "fwd" and last(rr).n == 1]}
    out = []
    for size in (1, 2, 65):
        for kind in ("rev", "fwd1"):
            if size == 1:
                idx = [next(i for i in head if i in tail[kind])]
            else:
                idx = [head[size % len(head)]] + [rng.randrange(len(pool)) for _ in range(size - 2)] + [tail[kind][size % len(tail[kind])]]
            out.append((size, kind, [pool[i] for i in idx], [recs[i] for i in idx]))
    return out


def test_stream_ends(B, O):
    """The stream is exactly as long as the contract says and lies between words that are all 0, then all 1: the records are the
    oracle's both times, so nothing outside the stream -- and nothing of its padding -- reaches a record."""
    import torch
    batches = _end_batches(O)
    below = beyond = behind = 0
    for size, kind, reads, recs in batches:
        nts = sum(len(r) for r in reads)
        last_word, q0 = (nts - 1) >> 4, 0
        wl = []
        for read, rr in zip(reads, recs):
            wl += [r.last_nt(q0) >> 4 for r in rr if r.strand]
            q0 += len(read)
        assert min(wl) < 7, (size, kind)  # the window begins before word 0
        below += 1
        beyond += max(wl) > last_word + 2       # ends beyond the two words behind the stream
        behind += any(last_word < w <= last_word + 2 for w in wl)  # ends inside them
    assert below == len(batches) and beyond >= 2 and behind >= 2, (below, beyond, behind)
    with B.BriskHip(K, M, 14) as ix:
        for size, kind, reads, recs in batches:
            want = sorted(r.key() for rr in recs for r in rr)
            for fill in (0, 0xffffffff):
                stream, offs = pack_stream(reads, fill)
                assert len(stream) == (int(offs[-1]) + 15) // 16 + 2
                PAD = 64
                host = np.concatenate([np.full(PAD, fill, np.uint32), stream, np.full(PAD, fill, np.uint32)])
                d_all = torch.from_numpy(host.view(np.int32)).cuda()
                d_starts = torch.from_numpy(offs).cuda()
                torch.cuda.synchronize()
                bound = ix.scan_bound(d_starts.data_ptr(), len(reads))
                got = scan_records(ix, d_all.data_ptr() + 4 * PAD, d_starts, len(reads), bound)
                assert got == want, (size, kind, hex(fill))
                assert np.array_equal(d_all.cpu().numpy().view(np.uint32), host)


def test_binned_layout(B, O, capfd):
    """The bench's route: insert_packed scans into per-partition bins and the overflow regions behind them.  Partitions few enough
    that some bin overflows; the index is the oracle's multiset."""
    reads = corner_reads(CORNER_SEED[14])
    # (256 bins of 56 records for this batch; one of this read's two records shares its partition with 17 others: 14 records lie
    # beyond that bin, which an overflow region of 17 still holds -- more, and the library hands the batch to the classic path)
    reads += [reads[0]] * 52
    want, nk, nb = O.count(reads, K, M, 14)
    old = os.environ.get("BRISK_TRACE")
    os.environ["BRISK_TRACE"] = "1"  # (read when a handle is created)
    try:
        ix = B.BriskHip(K, M, 14, part_bits=8)
    finally:
        if old is None:
            del os.environ["BRISK_TRACE"]
        else:
            os.environ["BRISK_TRACE"] = old
    with ix:
        d_packed, d_starts, offs = packed_on_device(ix, reads)
        capfd.readouterr()
        ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads))
        ix.sync()
        st = ix.stats()
        got = oracle.multiset_lines(*ix.enumerate(), K)
    lines = [l for l in capfd.readouterr().err.splitlines() if "binned scan of" in l]
    assert len(lines) == 1, lines
    beyond = int(lines[0].split(" records beyond their bins")[0].split()[-1])
    assert beyond > 0, lines
    assert (st["nb_kmers"], st["nb_buckets"]) == (nk, nb)
    assert got == want


def test_query_and_per_position_modes(B, O):
    """The other four bodies of 63/21: reads in query mode (get_packed) and per-position mode (get_kmers), and one long sequence, which
    is scanned in chunks, through insert, get and get_kmers."""
    import torch
    rng = random.Random(4)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    long_seq = rnd(70_000) + "A" * 200 + rnd(60_000) + "ACGTTGCA" * 40 + rnd(3 * 65536 - 130_520)
    reads = corner_reads(CORNER_SEED[14])
    seqs = reads[:200] + [long_seq]
    queries = reads[100:] + [long_seq[1000:150_000], revcomp(long_seq[60_000:140_000])]
    h = oracle_index(O, seqs, K, M, 14)
    want, alts, base = expected_all(O, h, queries, K, M)
    qf, qo = oracle.pack_reads(queries)
    want_sums = O.index_query_reads(h, qf, qo)
    O.index_free(h)
    with B.BriskHip(K, M, 14) as ix:
        ix.insert_reads(seqs)
        d_packed, d_starts, offs = packed_on_device(ix, queries)
        d_sums = torch.zeros(len(queries), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ix.get_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(queries), d_sums.data_ptr())
        ix.sync()
        assert d_sums.cpu().numpy().view(np.uint64).tolist() == want_sums.tolist()
        counts, found, got_base = ix.get_kmers(queries)
        assert np.array_equal(got_base, base)
        assert_slots(as_u16(counts, found), want, alts, "get_kmers")
