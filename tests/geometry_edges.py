"""The key-layout boundary geometries: the table, brisk_hip_create's layout formula restated in Python, and
the inputs and oracle-side expectations that tests/test_geometry_edges.py, tests/test_geometry_edges_cpu.py and
tests/geometry_edges_worker.py share.  Nothing here touches the device or the library under test.

An entry's key is [routing-id low bits : shift | compacted k-mer : 2(k-b) | idx' : 6]; it is stored in one 64-bit word when it has
at most 64 bits and in two otherwise, and it cannot have more than 128.  The rows sit where that layout, the record (1 to 4 words)
and the scan (k <= 32 or above, minimizer_idx classes or none) change their code path."""
import random
from collections import namedtuple

import numpy as np

import oracle
from test_gpu_parity import SPECIAL

Row = namedtuple("Row", "k m b part_bits key_bits key_words shift nw why")

TABLE = [
    Row(33, 11, 4, 0, 64, 1, 0, 2, "exactly one word; k > 32; class bit"),
    Row(32, 11, 3, 0, 64, 1, 0, 2, "exactly one word at k = 32 (min-queue, nlow = 32); ext_bits = 16"),
    Row(35, 13, 6, 0, 64, 1, 0, 2, "exactly one word, no classes"),
    Row(34, 11, 4, 0, 66, 2, 0, 2, "first two-word key"),
    Row(33, 11, 6, 6, 66, 2, 6, 2, "routing field straddles the word boundary (60 + 6)"),
    Row(37, 15, 10, 8, 72, 2, 12, 2, "straddle with a long field"),
    Row(31, 11, 4, 2, 66, 2, 6, 2, "straddle at k <= 32; four big partitions"),
    Row(63, 21, 2, 0, 128, 2, 0, 4, "the ceiling; nw = 4"),
    Row(63, 21, 4, 1, 128, 2, 4, 4, "requested part_bits = 1 becomes 4 in the adjustment loop"),
    Row(63, 5, 2, 0, 128, 2, 0, 4, "shortest minimizer with classes; super-k-mer span 121 nt"),
    Row(62, 21, 1, 0, 128, 2, 0, 4, "b = 1, even k"),
    Row(63, 31, 2, 0, 128, 2, 0, 3, "m = 31 at the ceiling"),
    Row(45, 27, 14, 0, 72, 2, 4, 2, "2k-m = 63: last span of the 128-bit record builder"),
    Row(44, 23, 12, 0, 70, 2, 0, 2, "2k-m = 65: first span of the 256-bit one"),
    Row(33, 31, 14, 0, 48, 1, 4, 1, "window of 3 k-mers, nw = 1, k > 32"),
    Row(12, 5, 1, 0, 28, 1, 0, 1, "smallest practical; nw = 1; classes"),
]

# what the last column claims, as predicates over layout(...) -- one per row, in the table's order
PROPERTY = [
    lambda L: L["key_bits"] == 64 and L["k"] > 32 and L["cls_bits"] == 1,
    lambda L: L["key_bits"] == 64 and L["k"] == 32 and L["min_queue"] and L["nlow"] == 32 and L["ext_bits"] == 16,
    lambda L: L["key_bits"] == 64 and L["cls_bits"] == 0,
    lambda L: L["key_bits"] in (65, 66) and L["key_words"] == 2 and L["shift"] == 0,
    lambda L: L["straddle"] and L["entry_bits"] == 60 and L["shift"] == 6,
    lambda L: L["straddle"] and L["shift"] >= 12,
    lambda L: L["straddle"] and L["k"] <= 32 and L["part_bits"] == 2,
    lambda L: L["key_bits"] == 128 and L["nw"] == 4 and L["adjusted"] == 0,
    lambda L: L["key_bits"] == 128 and L["requested_part_bits"] == 1 and L["part_bits"] == 4 and L["adjusted"] == 3,
    lambda L: L["key_bits"] == 128 and L["m"] == 5 and L["cls_bits"] == 1 and L["span"] == 121,
    lambda L: L["key_bits"] == 128 and L["b"] == 1 and L["k"] % 2 == 0,
    lambda L: L["key_bits"] == 128 and L["m"] == 31,
    lambda L: L["span"] == 63 and not L["wide_record"],
    lambda L: L["span"] == 65 and L["wide_record"],
    lambda L: L["k"] - L["m"] + 1 == 3 and L["nw"] == 1 and L["k"] > 32,
    lambda L: L["nw"] == 1 and L["cls_bits"] == 1 and L["key_words"] == 1,
]

# The corners of brisk_hip_create's envelope: 1 <= b <= m < k <= 63, m odd and at most 31, b <= 16,
# k - b >= 4, a key of at most 128 bits.  Same fields; every row is created with the default part_bits.
CORNERS = [
    Row(63, 31, 16, 0, 108, 2, 8, 3, "32-bit bucket ids under a two-word key"),
    Row(33, 17, 16, 0, 48, 1, 8, 2, "32-bit bucket ids, one word, k > 32"),
    Row(32, 31, 16, 0, 46, 1, 8, 1, "k = m + 1 at k = 32, nw = 1, b = 16"),
    Row(31, 15, 15, 0, 44, 1, 6, 1, "2b = 30, min-queue scan"),
    Row(47, 23, 15, 0, 76, 2, 6, 2, "b = 15, two words"),
    Row(20, 17, 16, 0, 22, 1, 8, 1, "k - b = 4 at b = 16"),
    Row(19, 15, 15, 0, 20, 1, 6, 1, "k - b = 4 at b = 15"),
    Row(9, 5, 5, 0, 14, 1, 0, 1, "k - b = 4, the smallest key"),
    Row(16, 15, 7, 0, 24, 1, 0, 1, "k = m + 1 with an extended routing id"),
    Row(63, 3, 2, 0, 128, 2, 0, 4, "m = 3 at the ceiling, window of 61"),
    Row(10, 3, 1, 0, 24, 1, 0, 1, "m = 3, small k"),
    Row(21, 3, 3, 0, 42, 1, 0, 2, "m = b: suff_reduc = 0, the class bit is the only extension"),
    Row(31, 1, 1, 0, 66, 2, 0, 2, "m = 1: eight partitions of thousands of entries, a window of 31"),
]

# (part_bits, ext_bits, cls_bits) of every corner, from the layout formula, and what the row is there for
CORNER_PROPERTY = [
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (24, 0, 0) and L["b"] == 16 and L["key_words"] == 2 and L["shift"] == 8,
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (24, 0, 0) and L["b"] == 16 and L["key_words"] == 1 and L["k"] > 32,
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (24, 0, 0) and L["k"] == L["m"] + 1 == 32 and L["nw"] == 1 and L["shift"] == 8,
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (24, 0, 0) and 2 * L["b"] == 30 and L["min_queue"] and L["shift"] == 6,
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (24, 0, 0) and L["b"] == 15 and L["key_words"] == 2,
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (24, 0, 0) and L["k"] - L["b"] == 4 and L["b"] == 16,
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (24, 0, 0) and L["k"] - L["b"] == 4 and L["b"] == 15,
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (10, 0, 0) and L["k"] - L["b"] == 4 and L["key_bits"] == 14,
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (24, 10, 0) and L["k"] == L["m"] + 1,
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (7, 3, 1) and L["m"] == 3 and L["key_bits"] == 128 and L["k"] - L["m"] + 1 == 61,
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (7, 5, 1) and L["m"] == 3 and L["nw"] == 1,
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (7, 1, 1) and L["m"] == L["b"] == 3 and (L["m"] - L["b"] + 1) // 2 == 0,
    lambda L: (L["part_bits"], L["ext_bits"], L["cls_bits"]) == (3, 1, 1) and L["m"] == 1 and L["k"] - L["m"] + 1 == 31,
]

SATURATE_ROWS = [0, 3, 4, 7]  # the 64-bit, 66-bit, straddling and 128-bit keys
SATURATE_CORNERS = [0, 11]  # (63, 31, 16) and (21, 3, 3)
SHARDED_CORNERS = [0, 3, 9]  # (63, 31, 16), (31, 15, 15), (63, 3, 2): the owner of a 32-bit, of a 30-bit and of an extended routing id
PERCALL_CORNERS = [1, 11]  # (33, 17, 16) and (21, 3, 3)
CLS_EXTRA = [Row(31, 11, 11, 0, 46, 1, 0, 2, "the class geometry of the other tests"), Row(63, 11, 4, 0, 124, 2, 0, 4, "classes under a two-word key")]


def row_id(r):
    return "k%dm%db%d" % (r.k, r.m, r.b) + ("-pb%d" % r.part_bits if r.part_bits else "")


def opts(r):
    return dict(part_bits=r.part_bits) if r.part_bits else {}


def layout(k, m, b, part_bits=0, cls_env=-1):
    """brisk_hip_create's geometry: None where it refuses (EUNSUPPORTED; EINVAL for k - b < 4).  cls_env: BRISK_CLS_BITS, -1 when unset."""
    w, kb = k - m, k - b
    if kb < 4:
        return None
    L = dict(k=k, m=m, b=b, requested_part_bits=part_bits, nw=(2 * (2 * k - m - b) + 63) // 64, ext_bits=0, cls_bits=0, cls_width=1)
    if not part_bits and 2 * b < 24:
        if 2 * m < 24 and w + 1 >= 8:
            L["cls_bits"] = min(cls_env, 3) if cls_env >= 0 else 1
        from_hash = min(24 - 2 * b, 2 * (m - b), 16 - L["cls_bits"])
        L["ext_bits"] = from_hash + L["cls_bits"]
        if L["cls_bits"]:
            L["cls_width"] = (w + 1 + (1 << L["cls_bits"]) - 1) >> L["cls_bits"]
    rbits = 2 * b + L["ext_bits"]
    part = min(part_bits, 2 * b) if part_bits else rbits if L["ext_bits"] else min(rbits, 24)  # an extended routing id is never cut
    shift, adjusted = rbits - part, 0
    while shift + 2 * kb + 6 > 128 and shift > 0:  # the key cannot have more than 128 bits: partitions get narrower instead
        shift, part, adjusted = shift - 1, part + 1, adjusted + 1
    if shift + 2 * kb + 6 > 128 or part > 30:
        return None
    entry_bits = 2 * kb + 6
    L.update(part_bits=part, shift=shift, adjusted=adjusted, entry_bits=entry_bits, key_bits=shift + entry_bits,
             key_words=1 if shift + entry_bits <= 64 else 2, straddle=entry_bits < 64 < entry_bits + shift, record_words=L["nw"] + 1,
             span=2 * k - m, wide_record=2 * k - m > 64, min_queue=k <= 32, nlow=min(32, k))
    return L


def row_layout(r, cls_env=-1):
    return layout(r.k, r.m, r.b, r.part_bits, cls_env)


def check_library_layout(r, lib_layout, info=None, cls_env=-1):
    """the library's own numbers (BriskHip.layout, snapshot_info of a file it saved) against the formula and the table"""
    L = row_layout(r, cls_env)
    for f in ("record_words", "part_bits", "ext_bits", "cls_bits", "cls_width"):
        assert lib_layout[f] == L[f], (row_id(r), f, lib_layout[f], L[f])
    if info is not None:
        for f in ("key_words", "shift", "part_bits", "ext_bits", "cls_bits", "cls_width"):
            assert info[f] == L[f], (row_id(r), f, info[f], L[f])
    if cls_env < 0:
        assert (L["key_bits"], L["key_words"], L["shift"], L["nw"]) == (r.key_bits, r.key_words, r.shift, r.nw), (row_id(r), L)
    return L


# ---- inputs: the smallest that still go wrong ---------------------------------------------------------------------------------
GLEN = 6000  # A is drawn from the first 4 kb of it, B from the last 4 kb: test_setops.two_samples (every row meets the bounds with it)
_cases = {}


def read_sets(r):
    """(A, B, C) of one geometry, seeded from (k, m, b): A ~400 reads of 150 nt from 4 kb, both strands, a third of them repeated,
    test_gpu_parity.SPECIAL and thirty ragged reads of 1..400 nt; B overlaps A (test_setops.two_samples); C goes in after a set
    operation (as test_setops.test_gets_and_inserts_after_an_operation builds it)."""
    from test_setops import two_samples
    seed = r.k * 10000 + r.m * 100 + r.b
    a, b = two_samples(seed, glen=GLEN, n_a=400, n_b=260)
    rng = random.Random(seed + 1)
    if r.m == 1:
        # A one-nucleotide minimizer ties at almost every window, so which (k-mer, minimizer_idx) a k-mer is stored under depends
        # on the read around it: two samples of one genome share next to nothing.  B takes whole reads of A instead -- every
        # second drawn read, with other repeat factors than A has -- and keeps its own reads of the genome's last third.
        own = [s for s in b[:260] if s not in a]
        b = a[0:400:2] + a[0:100:2] * 2 + own[:130] + own[:30] * 3 + SPECIAL * 2
    a = a + ["".join(rng.choice("ACGT") for _ in range(rng.randint(1, 400))) for _ in range(30)]
    if min(len(s) for s in a) >= r.k:  # k of 10 or less: the ragged reads happen to have none shorter than k
        a = a + ["".join(rng.choice("ACGT") for _ in range(n)) for n in (r.k - 1, r.k // 2, 1)]
    c = a[40:100] + b[10:60] + ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(40)]
    return a, b, c


def queries_of(reads_a, reads_b, reads_c, n_queries=(70, 50, 30)):
    """the reads a row is queried with: reads of A (present), of B (half of them absent), of C's random tail (absent), the
    low-complexity set"""
    na, nb_, nc = n_queries
    return [q.upper() for q in reads_a[:na] + reads_a[-12:] + reads_b[:nb_] + reads_c[-nc:] + SPECIAL]


# ---- the reference's own answers (tests/golden/envelope_reference.json, written by tests/golden/make_golden.py envelope) -----------
def all_rows():
    return TABLE + CORNERS


def sums_md5(sums):
    """md5 of per-read sums as little-endian uint64 words (make_golden.stream_md5 of one array)"""
    import hashlib
    return hashlib.md5(np.asarray(sums).astype("<u8").tobytes()).hexdigest()


def lines_md5(lines):
    """md5 of sorted "KMER idx count" lines as the text "KMER idx=N count\\n" (make_golden.md5_lines)"""
    import hashlib
    return hashlib.md5("".join("{} idx={} {}\n".format(*l.split()) for l in lines).encode()).hexdigest()


def envelope_answers(X, r):
    """What X (oracle.Oracle or oracle.Ref: the same calls) says about row r: the index of reads A, the per-read sums of the row's
    queries.  The record of envelope_reference.json."""
    a, b, c = read_sets(r)
    q = queries_of(a, b, c)
    flat, offs = oracle.pack_reads(a)
    qflat, qoffs = oracle.pack_reads(q)
    h = X.index_new(r.k, r.m, r.b)
    try:
        X.index_insert_reads(h, flat, offs)
        nb_kmers, nb_buckets = X.index_stats(h)
        lines = oracle.multiset_lines(*X.index_dump(h), r.k)
        sums = X.index_query_reads(h, qflat, qoffs)
    finally:
        X.index_free(h)
    return dict(k=r.k, m=r.m, b=r.b, nb_kmers=nb_kmers, nb_buckets=nb_buckets, md5=lines_md5(lines), sums_md5=sums_md5(sums))


class Case:
    """everything the oracle says about one row's inputs; computed once, shared, and left unchanged.  The three oracle indexes of a
    row (a few thousand entries each) are kept for the life of the process: the tests look entries up in them."""

    def __init__(self, O, r, n_queries=(70, 50, 30)):
        from test_kmer_query import expected_all
        from test_setops import as_dict
        from test_spectrum_prune import oracle_index
        k, m, b = r.k, r.m, r.b
        self.row = r
        self.reads_a, self.reads_b, self.reads_c = read_sets(r)
        self.ha, self.hb, self.hc = (oracle_index(O, x, k, m, b) for x in (self.reads_a, self.reads_b, self.reads_c))
        self.dump_a = O.index_dump(self.ha)
        self.da, self.db, self.dc = (as_dict(O.index_dump(h)) for h in (self.ha, self.hb, self.hc))
        self.stats_a = O.index_stats(self.ha)
        self.queries = queries_of(self.reads_a, self.reads_b, self.reads_c, n_queries)
        self.qflat, self.qoffs = oracle.pack_reads(self.queries)
        self.slots, self.alts, self.base = expected_all(O, self.ha, self.queries, k, m)
        self.sums = O.index_query_reads(self.ha, self.qflat, self.qoffs)
        self.ambiguous = np.zeros(len(self.slots), bool)
        for s0, e0, _ in self.alts:
            self.ambiguous[s0:e0] = True
        base = self.base.astype(np.int64)
        seg = lambda v: np.array([int(v[base[i]:base[i + 1]].astype(np.int64).sum()) for i in range(len(self.queries))], np.uint64)
        # a read is plain when no span of it reads the same on both strands and its oracle sum is the sum of its slots
        self.clean = seg(self.ambiguous) == 0
        self.plain = (seg(np.where(self.slots & 0x100, self.slots & 0xff, 0)) == self.sums) & self.clean

    def preconditions(self):
        """the non-vacuity conditions, from the oracle alone; returns the figures"""
        da, db = self.da, self.db
        shared = [x for x in da if x in db]
        union = len(da) + len(db) - len(shared)
        differ = sum(da[x] != db[x] for x in shared)
        cnt = self.dump_a[3]
        kept = int(((cnt >= 2) & (cnt <= 255)).sum())
        fig = dict(shared=len(shared), only_a=len(da) - len(shared), only_b=len(db) - len(shared), union=union, differ=differ,
                   ambiguous=float(self.ambiguous.mean()), plain=float(self.plain.mean()), entries=len(cnt), kept=kept)
        assert min(fig["shared"], fig["only_a"], fig["only_b"]) * 10 >= union, fig
        assert differ * 10 >= len(shared), fig
        assert fig["ambiguous"] < 0.2 and fig["plain"] > 0.8, fig
        assert kept * 10 >= len(cnt) and (len(cnt) - kept) * 10 >= len(cnt), fig
        found = (self.slots & 0x100) != 0
        assert found.any() and not found.all(), fig  # present and absent slots among the queries
        return fig


def case(O, r):
    if r not in _cases:
        _cases[r] = Case(O, r)
    return _cases[r]


def filtered_slots(c, lo, hi):
    """(slots, alts) of the index that keeps only the entries with lo <= count <= hi"""
    def f(v):
        cnt = v & 0xff
        return np.where(((v & 0x100) != 0) & (cnt >= lo) & (cnt <= hi), v, 0).astype(np.uint16)
    return f(c.slots), [(s, e, f(v)) for s, e, v in c.alts]


def resolved_slots(c, got):
    """The oracle's slots with every span that is its own reverse complement laid in the order `got` (uint16 slots of get_kmers) has
    it -- which must be one of the two the oracle allows (test_kmer_query.assert_slots) -- so that order-dependent results over
    the low-complexity reads (a profile's run, the trimmed interval) have an expectation too."""
    want = c.slots.copy()
    for s, e, alt in c.alts:
        if np.array_equal(got[s:e], alt):
            want[s:e] = alt
    return want


def record_elements(records, W, k, b):
    """[(compacted k-mer, bucket, idx')] of super-k-mer records (c words..., bucket, n, idx0): compacted_j = (C >> 2(n-1-j)) &
    ones(2(k-b)), idx'_j = idx0 + j (SuperKmerLight.hpp:98, 301-312)"""
    ones = (1 << (2 * (k - b))) - 1
    out = []
    for t in records:
        C = sum(w << (64 * i) for i, w in enumerate(t[: W - 1]))
        bucket, n, idx0 = t[W - 1:]
        assert C >> (2 * (k - b + n - 1)) == 0
        out += [((C >> (2 * (n - 1 - j))) & ones, bucket, idx0 + j) for j in range(n)]
    return out


def oracle_records(O, h, reads, r):
    """the oracle's records of `reads` as tuples (c words..., bucket, n, idx0), and the words of a record with its header"""
    out = []
    for s in reads:
        C, bucket, n, idx0 = O.records(h, s, r.k, r.m, r.b)
        for i in range(len(n)):
            out.append(tuple(int(x) for x in C[i]) + (int(bucket[i]), int(n[i]), int(idx0[i])))
    return out, row_layout(r)["record_words"]


def expected_file_entries(O, c, L):
    """What a snapshot of the index of reads A must hold, from the oracle's records alone: sorted
    (bucket, class of minimizer_idx, stored key, count) -- key = [bucket's low `shift` bits | compacted k-mer : 2(k-b) | idx' : 6],
    count = the instances of (bucket, compacted, idx') mod 256."""
    from collections import Counter
    r = c.row
    records, W = oracle_records(O, c.ha, c.reads_a, r)
    n = Counter(record_elements(records, W, r.k, r.b))
    sr, top = (r.m - r.b + 1) // 2, (1 << L["cls_bits"]) - 1
    low = (1 << L["shift"]) - 1
    out = []
    for (comp, bucket, idxp), cnt in n.items():
        assert idxp < 64
        key = ((bucket & low) << L["entry_bits"]) | (comp << 6) | idxp
        out.append((bucket, min((idxp - sr) // L["cls_width"], top) if top else 0, key, cnt & 0xff))
    return sorted(out)


def file_entries(blocks, L):
    """the same tuples read out of a parsed snapshot (tests/snapshot_reader.py): the bucket is the routing id -- partition number,
    then the key's leading `shift` bits -- without its ext_bits; the class is the routing id's low cls_bits"""
    part_of = np.concatenate([np.repeat(bk["partitions"], bk["counts"]) for bk in blocks]).tolist()
    keys = np.concatenate([bk["keys"] for bk in blocks])
    data = np.concatenate([bk["data"] for bk in blocks]).tolist()
    whole = [int(x) for x in keys[:, 0]] if keys.shape[1] == 1 else [int(lo) | (int(hi) << 64) for lo, hi in keys]  # low word first
    top = (1 << L["cls_bits"]) - 1
    out = []
    for p, key, cnt in zip(part_of, whole, data):
        rid = (p << L["shift"]) | (key >> L["entry_bits"])
        out.append((rid >> L["ext_bits"], rid & top, key, cnt))
    return sorted(out)


# ---- saturating counts: the construction of tests/test_saturate.py with a read repeated past 255 --------------------------------
def saturate_reads():
    """(B, other, one): saturate_worker.base_reads (303 windows of one locus: exact oracle counts below 256), test_saturate's second
    set that overlaps it, and the read that goes in 300 times (the last window: away from the entries whose sum crosses 255)"""
    import saturate_worker as S
    reads = S.base_reads()
    g2 = S.rand_seq(random.Random(808), 160)
    other = reads[:150] + [g2[o:o + 100] for o in range(0, 61, 4)] * 2
    return reads, other, reads[-1:]


def saturate_expectation(O, r):
    """{identity: count} of X = B twice and one read 300 times, of Y = other twice, both saturating; nb_buckets of X and of X | Y"""
    import saturate_worker as S
    reads, other, one = saturate_reads()
    k, m, b = r.k, r.m, r.b
    ca, nb_a = S.yardstick(O, "B", reads, k, m, b)
    c1, _ = S.yardstick(O, "last window", one, k, m, b)
    cb, _ = S.yardstick(O, "other", other, k, m, b)
    want_a = {x: S.clamp(2 * c + 300 * c1.get(x, 0)) for x, c in ca.items()}
    want_b = {x: S.clamp(2 * c) for x, c in cb.items()}
    assert set(c1) <= set(ca)
    return want_a, want_b, nb_a, S.nb_buckets(O, "union", reads + other, k, m, b)


def cls_rows():
    """the rows whose routing id carries minimizer_idx classes, and two geometries of the other tests that do"""
    return [r for r in TABLE if row_layout(r)["cls_bits"]] + CLS_EXTRA
