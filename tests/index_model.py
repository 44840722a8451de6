"""A host model of one index, and random sequences of the public operations over two handles.  No device is touched here:
tests/test_index_model_cpu.py checks the model and the sequences, tests/op_sequence_worker.py replays them on the device.

The model is a dict {(hi, lo, minimizer_idx): stored count byte} plus the count mode.  Every operation is restated from the
BriskHip docstrings (brisk_amd/hipapi.py) and DESIGN.md 4.r / 4.u / 4.w / 4.y / 4.z; nothing is taken from the library.  The only
route from reads to identities is the CPU oracle: batch_dump() is Oracle.index_dump of one batch in an index of its own.

Left out on purpose: reallocate_into, the entry-id API and the sharded paths (other identities or ownership; test_reallocate.py,
test_percall_edges.py and test_sharded*.py hold them), nb_skmers, largest_bucket and the order of an enumeration."""
import random
from collections import Counter

import numpy as np

GEOMETRIES = {"k63m21b14": ((63, 21, 14), {}),               # two-word keys, the lean first-fill route
              "k31m11b11": ((31, 11, 11), {}),               # a class bit in the routing id, 9-byte entries
              "k47m13b8-pb4": ((47, 13, 8), {"part_bits": 4})}  # 16 partitions of several table chunks
MODES = ("wrap", "saturate")
TABLE_CHUNK = 256  # JN_ENT of brisk_setops.hip: a partition of `other` above it is several table chunks of k_join / k_joint
# chosen on the CPU (tests/test_index_model_cpu.py: test_sequence_quality asserts what they were chosen for)
SEEDS = {("k63m21b14", "wrap"): (2, 11, 18), ("k63m21b14", "saturate"): (7, 9, 10), ("k31m11b11", "wrap"): (1, 2, 4), ("k31m11b11", "saturate"): (2, 3, 10),
         ("k47m13b8-pb4", "wrap"): (1, 4, 5), ("k47m13b8-pb4", "saturate"): (1, 2, 4)}
# what tests/op_sequence_worker.py replays under each kernel variant: one committed seed of each geometry, the count modes in turn
WORKER_CASES = [(2, "k63m21b14", "wrap"), (2, "k31m11b11", "saturate"), (1, "k47m13b8-pb4", "wrap")]

# operations per sequence (a hot burst adds up to two): a whole enumeration of an index of 2^24 partitions costs the library a 64 MB
# directory copy, 65 ms on an MI355X, and the replay makes one or two after every operation -- 24 keep such a case below 4 s
N_OPS = 24
PRUNE_WINDOWS = [(1, 1), (2, 255), (0, 0), (3, 9), (0, 255)]
RULES = ("left", "min", "max", "sum")
# (min_self, max_self, min_other, max_other, keep_absent): intersect(left), subtract, a prune, two mixed ones, min_other > max_other
JOINT_WINDOWS = [(0, 255, 0, 255, False), (0, 255, 1, 0, True), (2, 255, 0, 255, True), (2, 20, 0, 1, True), (1, 255, 3, 255, False), (1, 40, 9, 2, True)]
MUTATING = ("insert", "hot", "prune", "merge", "intersect", "subtract", "filter_joint", "clear")
TWO_INDEX = ("merge", "intersect", "subtract", "filter_joint")
REQUIRED_KINDS = {"insert", "insert/split1", "insert/split7", "insert/split64", "insert/immediate", "hot", "prune", "merge", "intersect", "subtract",
                  "filter_joint", "filter_joint/keep_absent", "filter_joint/empty_other_window", "swapped", "pending", "reload/compact", "reload/room",
                  "reopen", "clear", "walk"}
_RC = str.maketrans("ACGT", "TGCA")


# ---- the model -------------------------------------------------------------------------------------------------------------------------
class IndexModel:
    def __init__(self, mode, entries=None):
        assert mode in MODES
        self.mode = mode
        self.d = dict(entries or {})

    def _sum(self, c, d):
        return (c + d) & 0xff if self.mode == "wrap" else min(255, c + d)

    def copy(self):
        return IndexModel(self.mode, self.d)

    # -- mutating operations: each returns what the C-ABI returns (entries new, or entries removed)
    def insert(self, batch):
        """adds a batch ({identity: times seen, 1..255}): wrap (c + d) & 0xff -- an entry whose byte comes to 0 stays present --,
        saturate min(255, c + d).  Returns the entries that are new (brisk_hip_insert_reads itself returns nothing)."""
        new = 0
        for key, c in batch.items():
            new += key not in self.d
            self.d[key] = self._sum(self.d.get(key, 0), c)
        return new

    def merge(self, other):
        """self := self UNION other, counts of shared entries added under the mode's rule; a stored 0 of `other` arrives as 0"""
        assert other.mode == self.mode
        return self.insert(other.d)

    def _keep(self, pred):
        n = len(self.d)
        self.d = {key: c for key, c in self.d.items() if pred(key, c)}
        return n - len(self.d)

    def prune(self, lo, hi):
        lo, hi = min(lo, 255), min(hi, 255)
        return self._keep(lambda key, c: lo <= c <= hi)

    def intersect(self, other, rule="left"):
        assert other.mode == self.mode
        f = {"left": lambda a, b: a, "min": min, "max": max, "sum": self._sum}[rule]
        n = len(self.d)
        self.d = {key: f(c, other.d[key]) for key, c in self.d.items() if key in other.d}
        return n - len(self.d)

    def subtract(self, other):
        return self._keep(lambda key, c: key not in other.d)

    def filter_joint(self, other, window):
        lo, hi, olo, ohi = (min(v, 255) for v in window[:4])
        absent = bool(window[4])
        return self._keep(lambda key, c: lo <= c <= hi and (olo <= other.d[key] <= ohi if key in other.d else absent))

    def clear(self):
        self.d = {}

    def save(self):
        return dict(self.d)

    def load(self, snapshot):
        assert not self.d, "load takes an empty index"
        self.d = dict(snapshot)
        return len(self.d)

    # -- read-only
    def compare(self, other):
        shared = [key for key in self.d if key in other.d]
        return dict(both=len(shared), only_self=len(self.d) - len(shared), only_other=len(other.d) - len(shared),
                    sum_min=sum(min(self.d[x], other.d[x]) for x in shared), sum_self=sum(self.d[x] for x in shared), sum_other=sum(other.d[x] for x in shared))

    def joint_spectrum(self, other):
        from brisk_amd import joint_spectrum_from_entries  # the definition, host arithmetic only (as tests/test_joint.py uses it)
        return joint_spectrum_from_entries(self.dump(), other.dump())

    def dump(self, lo=0, hi=255):
        """(lo, hi, minimizer_idx, count) arrays as BriskHip.enumerate returns them, in no particular order; with bounds: that count
        range only"""
        keys = [key for key, c in self.d.items() if lo <= c <= hi] if (lo, hi) != (0, 255) else list(self.d)
        return (np.array([x[1] for x in keys], np.uint64), np.array([x[0] for x in keys], np.uint64), np.array([x[2] for x in keys], np.uint8),
                np.array([self.d[x] for x in keys], np.uint8))

    def spectrum(self):
        return np.bincount(np.fromiter(self.d.values(), np.int64, len(self.d)), minlength=256).astype(np.uint64)

    def stats(self, O, h):
        """(nb_kmers, nb_buckets); h: any oracle index of the geometry"""
        dump = self.dump()
        return len(self.d), len(np.unique(O.bucket_ids(h, dump[0], dump[1], dump[2])))

    def digest(self, O):
        return O.digest_entries(*self.dump())


def as_dict(dump):
    return {(h, l, i): c for l, h, i, c in zip(*(np.asarray(x).tolist() for x in dump))}


def rows(dump):
    """sorted (hi, lo, idx, cnt) rows: a multiset of entries as one array"""
    out = np.zeros(len(dump[0]), dtype=[("hi", np.uint64), ("lo", np.uint64), ("idx", np.uint8), ("cnt", np.uint8)])
    out["lo"], out["hi"], out["idx"], out["cnt"] = dump
    return out[np.lexsort((out["cnt"], out["idx"], out["lo"], out["hi"]))]


def diff_entries(got, want, limit=4):
    """the comparator: None when the enumerated multiset `got` is the model's (`want`: an IndexModel, or a dump of one), else a
    message naming what differs"""
    g, w = rows(got), rows(want.dump() if isinstance(want, IndexModel) else want)
    if len(g) == len(w) and np.array_equal(g, w):
        return None
    cg, cw = Counter(map(tuple, g.tolist())), Counter(map(tuple, w.tolist()))
    extra, missing = sorted((cg - cw).elements()), sorted((cw - cg).elements())
    return "entries differ: %d got, %d in the model; %d not in the model %s; %d not in the index %s (hi, lo, idx, count)" % (
        len(g), len(w), len(extra), extra[:limit], len(missing), missing[:limit])


# ---- from reads to identities: the oracle ------------------------------------------------------------------------------------------------
def batch_dump(O, reads, k, m, b):
    """{identity: times seen} of one batch: Oracle.index_dump of an index that received these reads alone.  The oracle's byte wraps
    silently, so the reads must hold no identity more than 255 times (check_batch)."""
    import oracle
    h = O.index_new(k, m, b)
    try:
        flat, offs = oracle.pack_reads(reads)
        O.index_insert_reads(h, flat, offs)
        return as_dict(O.index_dump(h))
    finally:
        O.index_free(h)


def check_batch(reads, k):
    """no canonical k-mer more than 255 times in the batch: an identity is a k-mer under one minimizer position, so this bounds it"""
    seen = Counter()
    for r in reads:
        for i in range(len(r) - k + 1):
            s = r[i:i + k]
            t = s[::-1].translate(_RC)
            seen[s if s < t else t] += 1
    worst = max(seen.values(), default=0)
    assert worst <= 255, ("a k-mer occurs %d times in one batch" % worst)
    return worst


# ---- the generator -----------------------------------------------------------------------------------------------------------------------
def make_case(seed, geometry, mode, n_ops=N_OPS):
    """One case: the batches (lists of reads; "hot" and "small" name the special ones), the create options of both handles and about
    n_ops operations over the handles A and B, as dicts.  Deterministic in (seed, geometry, mode)."""
    (k, m, b), opts = GEOMETRIES[geometry]
    rng = random.Random(seed * 1000003 + k * 1009 + m * 31 + b + (500 if mode == "saturate" else 0))
    glen = 6000
    genome = "".join(rng.choice("ACGT") for _ in range(glen))

    def read_at(lo, hi, L):
        p = rng.randrange(lo, hi - L + 1)
        s = list(genome[p:p + L])
        for i in range(L):
            if rng.random() < 0.01:  # a substitution: singletons exist
                s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
        s = "".join(s)
        return s[::-1].translate(_RC) if rng.random() < 0.5 else s

    def batch(n_reads):
        lo = rng.randrange(0, glen // 2)  # half of the genome: two batches share a part of their k-mers and differ in the rest
        out = [read_at(lo, lo + glen // 2, rng.randint(60, 150)) for _ in range(n_reads)]
        out += [read_at(lo, lo + glen // 2, rng.randint(1, k - 1)) for _ in range(3)] + [read_at(lo, lo + glen // 2, k) for _ in range(3)]
        if rng.random() < 0.5:  # low complexity, clipped: a homopolymer of 40 k-mers, periods 2 and 3 of 60
            out += [rng.choice("ACGT") * (k + 39), (rng.choice(["AC", "AG", "CT"]) * 80)[:k + 59], (rng.choice(["ACG", "AAT", "CTG"]) * 60)[:k + 59]]
        rng.shuffle(out)
        return out

    batches = [batch(rng.randint(100, 300)) for _ in range(8)]
    small = list(range(len(batches), len(batches) + 3))
    batches += [batch(rng.randint(3, 12)) for _ in small]
    hot = len(batches)
    starts = rng.sample(range(0, glen - 200, 200), 4)  # four reads that share no k-mer: 100 copies make a count of 100
    batches.append([genome[p:p + rng.randint(60, 150)] for p in starts] * 100)
    for reads in batches:
        check_batch(reads, k)

    immediate = {"A": rng.random() < 0.3, "B": rng.random() < 0.3}
    ops, forced = [], []
    other_of = {"A": "B", "B": "A"}

    def insert_op(h):
        return dict(op="insert", h=h, batch=rng.randrange(8), split=rng.choice([0, 0, 0, 1, 7, 64]))
    ops += [insert_op("A"), insert_op("B")]
    burst_at, burst_h = rng.randrange(4, n_ops - 12), rng.choice("AB")
    kinds = ["insert"] * 12 + ["hot"] * 2 + ["prune"] * 7 + ["merge"] * 8 + ["intersect"] * 9 + ["subtract"] * 6 + ["filter_joint"] * 10 + \
            ["reload"] * 6 + ["reopen"] * 3 + ["clear"] * 3 + ["walk"] * 5
    while len(ops) < n_ops:
        if len(ops) == burst_at:  # the hot batch three times in a row: 100, 200, 300 -- wrap and saturate part ways
            ops += [dict(op="hot", h=burst_h, batch=hot, split=0) for _ in range(3)]
            continue
        if forced:
            ops.append(insert_op(forced.pop()))
            continue
        kind, h = rng.choice(kinds), rng.choice("AAB")
        if kind == "insert":
            op = insert_op(h)
        elif kind == "hot":
            op = dict(op="hot", h=h, batch=hot, split=0)
        elif kind == "prune":
            lo, hi = rng.choice(PRUNE_WINDOWS)
            op = dict(op="prune", h=h, lo=lo, hi=hi)
            if (lo, hi) == (0, 0):
                forced.append(h)  # (nearly) everything goes: fill it again
        elif kind in TWO_INDEX:
            op = dict(op=kind, h=h, other=other_of[h], pending=rng.choice(small) if rng.random() < 0.4 else None)
            if kind == "intersect":
                op["rule"] = rng.choice(RULES)
            if kind == "filter_joint":
                op["window"] = rng.choice(JOINT_WINDOWS)
        elif kind == "reload":
            op = dict(op="reload", h=h, room=rng.random() < 0.4)
            if rng.random() < 0.7:
                forced.append(h)
        elif kind == "reopen":
            op = dict(op="reopen", h=h, room=rng.random() < 0.5, immediate=rng.random() < 0.3)
            if rng.random() < 0.7:
                forced.append(h)
        elif kind == "clear":
            op = dict(op="clear", h=h)
            forced.append(h)
        else:
            op = dict(op="walk", h=h)
        ops.append(op)
    return dict(seed=seed, geometry=geometry, mode=mode, kmb=(k, m, b), opts=dict(opts), genome=genome, batches=batches, hot=hot, small=small,
                immediate=immediate, ops=ops)


def describe(op):
    return " ".join("%s=%s" % (key, v) for key, v in op.items() if v is not None)


def op_kinds(case):
    """the kinds of operation a case holds, as REQUIRED_KINDS names them"""
    out, immediate = set(), dict(case["immediate"])
    for op in case["ops"]:
        name = op["op"]
        out.add(name if name not in ("reload",) else "reload/room" if op["room"] else "reload/compact")
        if name in ("insert", "hot"):
            if op["split"]:
                out.add("insert/split%d" % op["split"])
            if immediate[op["h"]]:
                out.add("insert/immediate")
        if name == "reopen":
            immediate[op["h"]] = op["immediate"]
        if name in TWO_INDEX:
            if op["h"] == "B":
                out.add("swapped")
            if op["pending"] is not None:
                out.add("pending")
        if name == "filter_joint":
            if op["window"][4]:
                out.add("filter_joint/keep_absent")
            if op["window"][2] > op["window"][3]:
                out.add("filter_joint/empty_other_window")
    return out


def case_dumps(O, case):
    k, m, b = case["kmb"]
    return [batch_dump(O, reads, k, m, b) for reads in case["batches"]]


def apply_op(op, models, dumps):
    """one operation on the models {"A": IndexModel, "B": IndexModel}; returns what the C-ABI call returns (None where it returns
    nothing: insert, clear, walk).  A pending insert into `other` goes first."""
    me = models[op["h"]]
    name = op["op"]
    if name in ("insert", "hot"):
        me.insert(dumps[op["batch"]])
        return None
    if name == "prune":
        return me.prune(op["lo"], op["hi"])
    if name in TWO_INDEX:
        other = models[op["other"]]
        if op["pending"] is not None:
            other.insert(dumps[op["pending"]])
        if name == "merge":
            return me.merge(other)
        if name == "subtract":
            return me.subtract(other)
        if name == "intersect":
            return me.intersect(other, op["rule"])
        return me.filter_joint(other, op["window"])
    if name in ("reload", "reopen"):  # save -> clear -> load, or save -> a new handle opened from the file: the entries are the same
        snap = me.save()
        me.clear()
        return me.load(snap)
    if name == "clear":
        me.clear()
        return None
    assert name == "walk", name
    return None


def run_model(case, dumps):
    """the case on the models alone: yields (index, op, return value, models) after every operation"""
    models = {"A": IndexModel(case["mode"]), "B": IndexModel(case["mode"])}
    for i, op in enumerate(case["ops"]):
        ret = apply_op(op, models, dumps)
        yield i, op, ret, models


# ---- probes: the lookup sample and the query reads of a case --------------------------------------------------------------------------------
def _codes(s):
    return (np.frombuffer(s.encode(), np.uint8) >> 1) & 3  # A0 C1 T2 G3


def _window_words(codes, k):
    """(lo, hi) of the k-mer at every position, first nucleotide most significant"""
    n = len(codes) - k + 1
    lo, hi = np.zeros(max(n, 0), np.uint64), np.zeros(max(n, 0), np.uint64)
    if n <= 0:
        return lo, hi
    c, nlo = codes.astype(np.uint64), min(k, 32)
    for i in range(k):
        if i >= k - nlo:
            lo |= c[i:i + n] << np.uint64(2 * (k - 1 - i))
        else:
            hi |= c[i:i + n] << np.uint64(2 * (k - nlo - 1 - i))
    return lo, hi


def slot_identities(O, reads, k, m):
    """The identity behind every get_kmers slot of `reads`, from the oracle's enumerator (as expected_slots of tests/test_kmer_query.py
    walks it): a list of (hi, lo, idx) per slot, base[n_reads + 1], and [(start, end)] for the vectors whose span is its own reverse
    complement -- there the slots may also hold the same values in reverse order."""
    ids, base, alts = [], [0], []
    for read in reads:
        codes = _codes(read)
        nk = max(len(codes) - k + 1, 0)
        if nk:
            f_lo, f_hi = _window_words(codes, k)
            r_lo, r_hi = _window_words((codes ^ 2)[::-1].copy(), k)
            r_lo, r_hi = r_lo[::-1], r_hi[::-1]
            _, skm_n, lo, hi, idx, _ = O.enumerate(read, k, m)
            p = t = 0
            for n in skm_n.tolist():
                vlo, vhi, vidx = lo[t:t + n], hi[t:t + n], idx[t:t + n]
                fwd = np.array_equal(vlo, f_lo[p:p + n]) and np.array_equal(vhi, f_hi[p:p + n])
                rev = np.array_equal(vlo, r_lo[p:p + n][::-1]) and np.array_equal(vhi, r_hi[p:p + n][::-1])
                assert fwd or rev, (read[:60], p, n)
                vec = list(zip(vhi.tolist(), vlo.tolist(), vidx.tolist()))
                ids += vec if fwd else vec[::-1]
                if fwd and rev:
                    alts.append((base[-1] + p, base[-1] + p + n))
                p, t = p + n, t + n
            assert p == nk
        base.append(base[-1] + nk)
    return ids, np.array(base, np.uint64), alts


def expected_slots(model, ids, alts):
    """uint16 per slot (0 absent, 0x100 | byte present) of the model, and the alternatives in the form assert_slots takes"""
    d = model.d
    want = np.array([0x100 | d[x] if x in d else 0 for x in ids], np.uint16)
    return want, [(s, e, want[s:e][::-1].copy()) for s, e in alts]


def case_probes(O, case, dumps, n_lookup=2000, n_query=60):
    """Fixed per case: a lookup sample of n_lookup identities out of everything the case ever inserts, and of a batch it never
    inserts; n_query query reads (inserted ones, never inserted ones, a short one and one of exactly k) with their slot identities."""
    k, m, b = case["kmb"]
    rng = random.Random(case["seed"] * 77 + 5)
    used = sorted({op["batch"] for op in case["ops"] if "batch" in op} | {op["pending"] for op in case["ops"] if op.get("pending") is not None})
    inserted = sorted(set().union(*(dumps[i].keys() for i in used)))
    stranger = "".join(rng.choice("ACGT") for _ in range(3000))
    never_reads = [stranger[p:p + 150] for p in range(0, 2850, 50)]
    never = sorted(set(batch_dump(O, never_reads, k, m, b)) - set(inserted))
    sample = rng.sample(inserted, min(len(inserted), n_lookup - 300)) + rng.sample(never, min(len(never), 300))
    pool = [r for i in used for r in case["batches"][i][:40] if len(r) > k]
    queries = rng.sample(pool, n_query - 12) + rng.sample(never_reads, 10) + [pool[0][:k - 1], pool[1][:k]]
    ids, base, alts = slot_identities(O, queries, k, m)
    return dict(sample=sample, sample_lo=np.array([x[1] for x in sample], np.uint64), sample_hi=np.array([x[0] for x in sample], np.uint64),
                sample_idx=np.array([x[2] for x in sample], np.uint8), queries=queries, slot_ids=ids, base=base, alts=alts)
