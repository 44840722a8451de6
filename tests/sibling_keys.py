"""Sibling keys ("sibling keys"): pairs of reads whose super-k-mer records are equal word for word -- the same
compacted string, the same number of k-mers, the same idx' -- and differ in the bucket alone.  Nothing here touches the device or
the library under test; every pair is accepted by the oracle's records (Oracle.records), never by the library.

An entry's stored key is [bucket's low `shift` bits | compacted k-mer : 2(k-b) | idx' : 6] and its partition is bucket >> shift
(geometry_edges.layout).  The bucket is the bit field [2sr, 2sr + 2b) of the minimizer's hash, sr = ceil((m-b)/2), and the hash
replaces the minimizer in place through an invertible mixer (bo_mix / bo_mix_inv).  So: take a random read that is one
super-k-mer, flip bits of that field in the hash of its minimizer, invert the mixer, and write the m-mer back where the minimizer
stands, on its strand.  The oracle accepts the pair when both reads give one record each with the same C, n and idx0 and buckets
that differ by exactly the flipped bits (the new m-mer must again be the canonical minimizer of every k-mer of the read).

  sibling  the buckets differ inside the low `shift` bits only: same partition, keys that differ in the routing field alone.
           "bits" names the differing bits; one bit t < shift, or two and more (several hash bits flipped at once).
  cousin   the buckets differ in exactly one bit at or above `shift`: the same key in another partition.  The control, and the
           only class where shift = 0.
  single   reads of k nucleotides, one k-mer;  record: reads of k + 7 (one super-k-mer of 8 k-mers; k + k - m where the window
           holds fewer than 8 k-mers), the whole record equal apart from the bucket.

Where the routing field lies across the two key words (layout["straddle"]) a pair is tagged with the word its differing bits lie
in: "low", "high", or "both" for a multi-bit pair on either side."""
import gzip
import json
import os
import random
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (run as a script, to write the fixture)
    sys.path.insert(0, ROOT)
import oracle
from geometry_edges import TABLE, layout

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sibling_pairs.json.gz")
LIMIT = 200000  # candidate reads per geometry
_RC = str.maketrans("ACGT", "TGCA")

Geo = namedtuple("Geo", "k m b part_bits kind")  # kind: "body" (a compile-time kernel body), "straddle", "row" (another table row), "cousins" (shift = 0)

# the eight geometries with compile-time insert and query bodies: <3,49,4..1>, <2,17,4..6>, <2,20,0>
BODIES = [Geo(63, 21, 14, pb, "body") for pb in (0, 25, 26, 27)] + [Geo(31, 15, 14, pb, "body") for pb in (0, 23, 22)] + [Geo(31, 11, 11, 0, "cousins")]
STRADDLE = {(33, 11, 6, 6), (37, 15, 10, 8), (31, 11, 4, 2)}
ROWS = [Geo(r.k, r.m, r.b, r.part_bits, "straddle" if (r.k, r.m, r.b, r.part_bits) in STRADDLE else "row") for r in TABLE if r.shift > 0]
COUSIN_ROWS = [Geo(33, 11, 4, 0, "cousins"), Geo(34, 11, 4, 0, "cousins")]
GEOMETRIES = BODIES + ROWS + COUSIN_ROWS

# what find_pairs collects: (singles, records) per sibling bit, of multi-bit siblings, of cousins
PER_BIT, MULTI, COUSINS = (8, 4), (8, 4), (8, 4)


def geo_id(g):
    return "k%dm%db%d" % (g.k, g.m, g.b) + ("-pb%d" % g.part_bits if g.part_bits else "")


def geo_seed(g):
    return ((g.k * 100 + g.m) * 100 + g.b) * 100 + g.part_bits


def geo_layout(g):
    return layout(g.k, g.m, g.b, g.part_bits)


def record_len(k, m):
    """nucleotides of a "record" read: 8 k-mers, or the whole window where it holds fewer (k33 m31: 3)"""
    return k + min(7, k - m)


def revcomp(s):
    return s[::-1].translate(_RC)


def word_side(L, bits):
    """the key word(s) the routing bits `bits` are stored in: bit t of the field is bit entry_bits + t of the key"""
    sides = {"low" if L["entry_bits"] + t < 64 else "high" for t in bits}
    return sides.pop() if len(sides) == 1 else "both"


def one_record(O, h, read, k, m, b):
    """(C words, bucket, n, idx0) when `read` is one super-k-mer, else None"""
    C, bucket, n, idx0 = O.records(h, read, k, m, b)
    if len(n) != 1 or int(n[0]) != len(read) - k + 1:
        return None
    return tuple(int(x) for x in C[0]), int(bucket[0]), int(n[0]), int(idx0[0])


def primed(O, read, k, m, b, mask):
    """`read` (one super-k-mer) with the bucket bits `mask` of its minimizer's hash flipped, in the super-k-mer's orientation; None
    where the minimizer cannot be located as an m-mer of the read"""
    _, skm_n, lo, hi, idx, _ = O.enumerate(read, k, m)
    if len(skm_n) != 1:
        return None
    ks, at = oracle.kmer2str(lo[0], hi[0], k), int(idx[0])  # element 0 in the minimizer's orientation; its m-mer ends `at` nts from the end
    t = read if ks in read else revcomp(read)
    p = t.find(ks)
    if p < 0:
        return None
    q = p + k - at - m
    mm = oracle.str2kmer(t[q:q + m])[0]
    sr = (m - b + 1) // 2
    new = O.mix_inv(O.mix(mm, m) ^ (mask << (2 * sr)), m)
    return t[:q] + oracle.kmer2str(new, 0, m) + t[q + m:]


def _targets(L, b):
    """[(class, size, bits or None)] -> wanted pairs, in the order they are filled"""
    shift = L["shift"]
    out = []
    for si, size in enumerate(("single", "record")):
        out += [(("sibling", size, (t,)), PER_BIT[si]) for t in range(shift)]
        if shift >= 2:
            out.append((("sibling", size, None), MULTI[si]))
        out.append((("cousin", size, None), COUSINS[si]))
    return out


def find_pairs(O, k, m, b, part_bits=0, seed=0, limit=LIMIT):
    """(pairs, candidates): the pairs of one geometry, dicts {cls, size, bits, a, b[, word]}, and the candidate reads drawn.
    Deterministic in its arguments.  A target that `limit` candidates do not fill stays short: the caller's floors decide."""
    L = layout(k, m, b, part_bits)
    shift, low = L["shift"], (1 << L["shift"]) - 1
    rng = random.Random(seed)
    h = O.index_new(k, m, b)
    pairs, tried = [], 0
    try:
        for (cls, size, bits), want in _targets(L, b):
            n_nt = k if size == "single" else record_len(k, m)
            got = 0
            while got < want and tried < limit:
                tried += 1
                read = "".join(rng.choice("ACGT") for _ in range(n_nt))
                if cls == "cousin":
                    mask = 1 << rng.randrange(shift, 2 * b)
                elif bits is not None:
                    mask = 1 << bits[0]
                else:
                    mask = rng.randrange(1, 1 << shift)
                    if bin(mask).count("1") < 2:
                        continue
                ra = one_record(O, h, read, k, m, b)
                if ra is None:
                    continue
                other = primed(O, read, k, m, b, mask)
                rb = other and one_record(O, h, other, k, m, b)
                if not rb or (ra[0], ra[2], ra[3]) != (rb[0], rb[2], rb[3]) or ra[1] ^ rb[1] != mask:
                    continue
                diff = [t for t in range(2 * b) if mask >> t & 1]
                pair = dict(cls=cls, size=size, bits=diff, a=read, b=other)
                if L["straddle"] and cls == "sibling":
                    pair["word"] = word_side(L, diff)
                pairs.append(pair)
                got += 1
    finally:
        O.index_free(h)
    return pairs, tried


def verify_pair(O, h, g, L, pair):
    """a committed pair against the oracle's records: the figures of find_pairs' acceptance, recomputed"""
    k, m, b = g.k, g.m, g.b
    ra, rb = one_record(O, h, pair["a"], k, m, b), one_record(O, h, pair["b"], k, m, b)
    assert ra and rb, (geo_id(g), pair)
    assert len(pair["a"]) == len(pair["b"]) == (k if pair["size"] == "single" else record_len(k, m)), (geo_id(g), pair)
    assert ra[2] == rb[2] == len(pair["a"]) - k + 1
    assert (ra[0], ra[2], ra[3]) == (rb[0], rb[2], rb[3]), (geo_id(g), "the records differ beyond the bucket", pair)
    d, low = ra[1] ^ rb[1], (1 << L["shift"]) - 1
    assert d and [t for t in range(2 * b) if d >> t & 1] == pair["bits"], (geo_id(g), d, pair)
    if pair["cls"] == "sibling":
        assert d & ~low == 0 and ra[1] >> L["shift"] == rb[1] >> L["shift"], (geo_id(g), pair)  # same partition, the field differs
        if L["straddle"]:
            assert pair["word"] == word_side(L, pair["bits"])
    else:
        assert d & low == 0 and bin(d).count("1") == 1, (geo_id(g), pair)  # the same field: the same key in another partition
    return ra, rb


def tally(L, pairs):
    """{(class, size, bits as a tuple | "multi" | "any"): pairs}, and for straddling layouts {(size, word): sibling pairs}"""
    n, words = {}, {}
    for p in pairs:
        key = "any" if p["cls"] == "cousin" else tuple(p["bits"]) if len(p["bits"]) == 1 else "multi"
        n[(p["cls"], p["size"], key)] = n.get((p["cls"], p["size"], key), 0) + 1
        if "word" in p:
            words[(p["size"], p["word"])] = words.get((p["size"], p["word"]), 0) + 1
    return n, words


def generate(O):
    out = {}
    for g in GEOMETRIES:
        pairs, tried = find_pairs(O, g.k, g.m, g.b, g.part_bits, geo_seed(g))
        out[geo_id(g)] = dict(k=g.k, m=g.m, b=g.b, part_bits=g.part_bits, seed=geo_seed(g), candidates=tried, pairs=pairs)
    return out


def load_fixture():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


# ---- the read sets of the device tests, and what the oracle says about them -----------------------------------------------------------
def read_sets(g, pairs):
    """(X, Y, background): X = every unprimed member, singles three times and records twice, and 100 random 150-nt reads; Y = every
    primed member once and 30 of the same background reads"""
    rng = random.Random(geo_seed(g) + 7)
    bg = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(100)]
    x = [p["a"] for p in pairs for _ in range(3 if p["size"] == "single" else 2)] + bg
    y = [p["b"] for p in pairs] + bg[:30]
    rng.shuffle(x)
    rng.shuffle(y)
    return x, y, bg


class Case:
    """Everything the oracle says about one geometry's read sets; computed once per process, shared and left unchanged.
    queries: every primed member (pair order), every unprimed member, ten background reads of both sets and five of X alone."""

    def __init__(self, O, g, pairs):
        from index_model import batch_dump, slot_identities
        from test_kmer_query import expected_all, oracle_index
        k, m, b = g.k, g.m, g.b
        self.g, self.L, self.pairs = g, geo_layout(g), pairs
        self.x, self.y, self.bg = read_sets(g, pairs)
        self.dx, self.dy = batch_dump(O, self.x, k, m, b), batch_dump(O, self.y, k, m, b)
        self.ids_a = [sorted(batch_dump(O, [p["a"]], k, m, b)) for p in pairs]  # the identities (hi, lo, minimizer_idx) of each member
        self.ids_b = [sorted(batch_dump(O, [p["b"]], k, m, b)) for p in pairs]
        self.hx = oracle_index(O, self.x, k, m, b)  # kept for the life of the process
        self.queries = [p["b"] for p in pairs] + [p["a"] for p in pairs] + self.bg[:10] + self.bg[95:]
        self.qflat, self.qoffs = oracle.pack_reads(self.queries)
        self.sums_x = O.index_query_reads(self.hx, self.qflat, self.qoffs)
        self.slots_x, self.alts_x, self.base = expected_all(O, self.hx, self.queries, k, m)
        self.slot_ids, base, self.alt_spans = slot_identities(O, self.queries, k, m)
        assert base.tolist() == self.base.tolist()

    def model(self, mode, *batches):
        """the index that received `batches` (dicts of batch_dump) in turn: tests/index_model.py"""
        from index_model import IndexModel
        mod = IndexModel(mode)
        for d in batches:
            mod.insert(d)
        return mod

    def preconditions(self):
        """from the oracle alone: each pair is two sets of identities, as many as the read has k-mers, that share nothing; X holds
        the unprimed one with count 3 or 2 and nothing of the primed one, Y the reverse with count 1; a read of a primed member finds
        nothing in the index of X -- an index that dropped the routing field from the key would find the unprimed member's entries"""
        n = len(self.pairs)
        for i, p in enumerate(self.pairs):
            a, b = self.ids_a[i], self.ids_b[i]
            assert len(a) == len(b) == len(p["a"]) - self.g.k + 1 and not set(a) & set(b), p
            assert all(self.dx[x] == (3 if p["size"] == "single" else 2) and x not in self.dy for x in a), p
            assert all(self.dy[x] == 1 and x not in self.dx for x in b), p
            assert int(self.sums_x[i]) == 0 and not self.slots_x[int(self.base[i]):int(self.base[i + 1])].any(), p
            assert int(self.sums_x[n + i]) == len(a) * self.dx[a[0]], p
        shared = [x for x in self.dx if x in self.dy]
        assert len(shared) > 1000 and all(self.dx[x] == self.dy[x] == 1 for x in shared)  # the thirty background reads
        return dict(pairs=n, entries_x=len(self.dx), entries_y=len(self.dy), shared=len(shared))

    def file_keys(self, O, i):
        """[(partition, stored key)] of the entries of pair i's two members, from the oracle's records:
        key = [bucket's low `shift` bits | compacted k-mer | idx'], partition = bucket >> shift.  Only where the routing id is the
        bucket (no ext_bits: every geometry with shift > 0)."""
        from geometry_edges import record_elements
        g, L = self.g, self.L
        assert L["ext_bits"] == 0
        out = []
        for read in (self.pairs[i]["a"], self.pairs[i]["b"]):
            C, bucket, n, idx0 = O.records(self.hx, read, g.k, g.m, g.b)
            recs = [tuple(int(w) for w in C[j]) + (int(bucket[j]), int(n[j]), int(idx0[j])) for j in range(len(n))]
            out.append([(bk >> L["shift"], ((bk & ((1 << L["shift"]) - 1)) << L["entry_bits"]) | (comp << 6) | idxp)
                        for comp, bk, idxp in record_elements(recs, L["record_words"], g.k, g.b)])
        return out


_cases = {}


def case(O, g):
    if g not in _cases:
        _cases[g] = Case(O, g, load_fixture()[geo_id(g)]["pairs"])
    return _cases[g]


if __name__ == "__main__":  # python tests/sibling_keys.py: writes the fixture anew (a few seconds of CPU time)
    import time
    oracle.build(ref=False)
    O = oracle.Oracle()
    t0 = time.time()
    data = generate(O)
    for gid, d in data.items():
        g = Geo(d["k"], d["m"], d["b"], d["part_bits"], "")
        n, words = tally(geo_layout(g), d["pairs"])
        print(gid, "shift", geo_layout(g)["shift"], "candidates", d["candidates"], {"%s/%s/%s" % (c, s, "".join(map(str, t)) if isinstance(t, tuple) else t): v for (c, s, t), v in sorted(n.items(), key=str)}, words)
    with gzip.GzipFile(FIXTURE, "wb", mtime=0) as f:
        f.write(json.dumps(data, sort_keys=True, separators=(",", ":")).encode())
    print("%s: %d bytes, %.0f s" % (FIXTURE, os.path.getsize(FIXTURE), time.time() - t0))
