"""CPU: the host model of tests/index_model.py against the oracle and the host definitions, the quality of every committed
operation sequence, and the comparator's ability to fail.  What the device does with the sequences is tests/test_op_sequences.py."""
import functools

import numpy as np
import pytest

import oracle
from index_model import (GEOMETRIES, JOINT_WINDOWS, MODES, MUTATING, N_OPS, REQUIRED_KINDS, SEEDS, TABLE_CHUNK, TWO_INDEX, IndexModel, apply_op, batch_dump,
                         case_dumps, case_probes, diff_entries, make_case, op_kinds, run_model)

CASES = [(g, mode, seed) for g in GEOMETRIES for mode in MODES for seed in SEEDS[g, mode]]
CASE_IDS = ["%s-%s-%d" % c for c in CASES]
A = 256


@functools.lru_cache(maxsize=None)
def _case(geometry, mode, seed):
    O = _oracle()
    case = make_case(seed, geometry, mode)
    return case, case_dumps(O, case)


@functools.lru_cache(maxsize=None)
def _oracle():
    oracle.build(ref=False)
    return oracle.Oracle()


def oracle_dump(O, reads, kmb):
    return batch_dump(O, reads, *kmb)


# ---- the model against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry,seed", [(g, seed) for g in GEOMETRIES for seed in SEEDS[g, "wrap"]])
def test_insert_only_prefix_equals_one_oracle_index(O, geometry, seed):
    """wrap mode: the model after the inserts that open a sequence is the oracle's one index of the same reads"""
    case, dumps = _case(geometry, "wrap", seed)
    for h in "AB":
        model, reads = IndexModel("wrap"), []
        for op in case["ops"]:
            if op["op"] not in ("insert", "hot"):
                break
            if op["h"] == h:
                model.insert(dumps[op["batch"]])
                reads += case["batches"][op["batch"]]
        assert reads
        assert model.d == oracle_dump(O, reads, case["kmb"]), (geometry, seed, h)
    # and further than the prefix goes: every batch of the case, the hot one three times -- counts wrap in the oracle as in the model
    model, reads = IndexModel("wrap"), []
    for i in list(range(len(case["batches"]))) + [case["hot"]] * 2:
        model.insert(dumps[i])
        reads += case["batches"][i]
    want = oracle_dump(O, reads, case["kmb"])
    assert model.d == want and max(dumps[case["hot"]].values()) >= 100 and min(want.values()) >= 0


def test_merge_of_two_dumps_is_the_dump_of_the_concatenated_reads(O):
    for geometry in GEOMETRIES:
        case, dumps = _case(geometry, "wrap", SEEDS[geometry, "wrap"][0])
        a_reads = case["batches"][0] + case["batches"][case["hot"]] * 2
        b_reads = case["batches"][1] + case["batches"][case["hot"]]
        a, b = IndexModel("wrap", oracle_dump(O, a_reads, case["kmb"])), IndexModel("wrap", oracle_dump(O, b_reads, case["kmb"]))
        want = oracle_dump(O, a_reads + b_reads, case["kmb"])
        new = a.merge(b)
        assert a.d == want and new == len(want) - len(oracle_dump(O, a_reads, case["kmb"]))
        assert any(c < 100 for key, c in want.items() if key in dumps[case["hot"]])  # 300 wrapped to 44 (+ what the batches add)


def test_saturating_sums():
    a, b = IndexModel("saturate", {(0, 1, 0): 200, (0, 2, 0): 255, (0, 3, 0): 7}), IndexModel("saturate", {(0, 1, 0): 100, (0, 2, 0): 1, (0, 4, 0): 255})
    w = IndexModel("wrap", a.d)
    x = a.copy()
    assert x.merge(b) == 1 and x.d == {(0, 1, 0): 255, (0, 2, 0): 255, (0, 3, 0): 7, (0, 4, 0): 255}
    w.merge(IndexModel("wrap", b.d))
    assert w.d == {(0, 1, 0): 44, (0, 2, 0): 0, (0, 3, 0): 7, (0, 4, 0): 255}  # a wrapped 0 stays present
    x = a.copy()
    assert x.intersect(b, "sum") == 1 and x.d == {(0, 1, 0): 255, (0, 2, 0): 255}
    assert w.prune(1, 300) == 1 and (0, 2, 0) not in w.d  # a bound above 255 means 255; the stored byte is compared


# ---- the model against the host definitions ------------------------------------------------------------------------------------------------
def two_models(O, geometry, mode):
    case, dumps = _case(geometry, mode, SEEDS[geometry, mode][0])
    a, b = IndexModel(mode), IndexModel(mode)
    for i in (0, 1, case["hot"], case["hot"], case["hot"]):
        a.insert(dumps[i])
    for i in (1, 2, case["hot"]):
        b.insert(dumps[i])
    return a, b


@pytest.mark.parametrize("mode", MODES)
def test_joint_spectrum_marginals_and_compare(O, mode):
    a, b = two_models(O, "k31m11b11", mode)
    J = a.joint_spectrum(b)
    assert np.array_equal(J[:A].sum(axis=1), a.spectrum()) and np.array_equal(J[:, :A].sum(axis=0), b.spectrum()) and J[A, A] == 0
    block, n = J[:A, :A].astype(object), np.arange(256, dtype=object)
    assert a.compare(b) == dict(both=int(block.sum()), only_self=int(J[:A, A].sum()), only_other=int(J[A, :A].sum()), sum_min=int((block * np.minimum.outer(n, n)).sum()),
                                sum_self=int((block.sum(axis=1) * n).sum()), sum_other=int((block.sum(axis=0) * n).sum()))
    assert a.compare(b)["both"] > 100 and a.compare(b)["only_self"] > 100 and a.compare(b)["only_other"] > 100
    assert bool(J[255].any()) == (mode == "saturate")  # the hot batch three times in a: 255 where counts stop, 300 - 256 + ... where they wrap


@pytest.mark.parametrize("mode", MODES)
def test_three_windows_are_intersect_subtract_and_prune(O, mode):
    a, b = two_models(O, "k63m21b14", mode)
    for window, same in (((0, 255, 0, 255, False), lambda x: x.intersect(b, "left")), ((0, 255, 1, 0, True), lambda x: x.subtract(b)),
                         ((2, 255, 0, 255, True), lambda x: x.prune(2, 255)), ((3, 9, 0, 255, True), lambda x: x.prune(3, 9))):
        x, y = a.copy(), a.copy()
        n = x.filter_joint(b, window)
        assert n == same(y) and x.d == y.d and 0 < n < len(a.d), window
    for window in JOINT_WINDOWS:  # and every window of the generator against the matrix: what stays is the sum of the bins that pass
        x, J = a.copy(), a.joint_spectrum(b)
        lo, hi, olo, ohi, absent = window
        x.filter_joint(b, window)
        assert len(x.d) == int(J[lo:hi + 1, olo:ohi + 1].sum()) + (int(J[lo:hi + 1, A].sum()) if absent else 0), window


# ---- the sequences ------------------------------------------------------------------------------------------------------------------------
def sequence_facts(O, case, dumps):
    """the case on the model, next to a shadow model in the other count mode"""
    (k, m, b), mode = case["kmb"], case["mode"]
    shadow = {h: IndexModel(MODES[1 - MODES.index(mode)]) for h in "AB"}
    h_any = O.index_new(k, m, b)
    f = dict(mutating=0, changed=0, diverged=False, refilled=False, compact_then_insert=False, big_partition=0, first_divergence=None)
    emptied, loaded = set(), set()
    before = {"A": {}, "B": {}}
    for i, op, ret, models in run_model(case, dumps):
        apply_op(op, shadow, dumps)
        h, name = op["h"], op["op"]
        now = models[h].d
        if name in MUTATING:
            f["mutating"] += 1
            f["changed"] += now != before[h]
        if name in ("insert", "hot"):
            f["refilled"] |= h in emptied and len(now) > 0
            f["compact_then_insert"] |= h in loaded
            emptied.discard(h)
        elif name in MUTATING and before[h] and not now:
            emptied.add(h)
        loaded.discard(h)
        if name in ("reload", "reopen") and not op["room"] and now:
            loaded.add(h)
        if name in TWO_INDEX and case["opts"].get("part_bits") and models[op["other"]].d:
            d = models[op["other"]].dump()
            ids = O.bucket_ids(h_any, d[0], d[1], d[2]).astype(np.int64) >> (2 * b - case["opts"]["part_bits"])
            f["big_partition"] = max(f["big_partition"], int(np.bincount(ids).max()))
        if not f["diverged"] and any(models[x].d != shadow[x].d for x in "AB"):
            f["diverged"], f["first_divergence"] = True, (i, h, models[h].copy(), shadow[h].copy())
        before = {x: dict(models[x].d) for x in "AB"}
    O.index_free(h_any)
    return f


@pytest.mark.parametrize("geometry,mode,seed", CASES, ids=CASE_IDS)
def test_sequence_quality(O, geometry, mode, seed):
    case, dumps = _case(geometry, mode, seed)
    f = sequence_facts(O, case, dumps)
    assert N_OPS <= len(case["ops"]) <= N_OPS + 2
    assert 3 * f["changed"] >= 2 * f["mutating"], f  # at least two thirds of the mutating operations change the model
    assert f["diverged"], "no count crosses 255: wrap and saturate agree all the way"
    assert f["refilled"], "no index becomes empty and is filled again"
    assert f["compact_then_insert"], "no compact load is followed by an insert"
    if case["opts"].get("part_bits") == 4:
        assert f["big_partition"] > TABLE_CHUNK, f["big_partition"]  # `other` of a two-index operation: several table chunks of k_join


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("mode", MODES)
def test_every_kind_occurs_across_the_seeds(geometry, mode):
    seen = set().union(*(op_kinds(_case(geometry, mode, seed)[0]) for seed in SEEDS[geometry, mode]))
    assert seen >= REQUIRED_KINDS, sorted(REQUIRED_KINDS - seen)


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_probes(O, geometry):
    """the lookup sample holds inserted and never inserted identities; the slots with a reverse-order alternative are at most 1 %"""
    for mode in MODES:
        for seed in SEEDS[geometry, mode]:
            case, dumps = _case(geometry, mode, seed)
            p = case_probes(O, case, dumps)
            n_slots = int(p["base"][-1])
            assert len(p["sample"]) == len(set(p["sample"])) >= 1500 and len(p["queries"]) == 60 and n_slots > 1500
            assert sum(e - s for s, e in p["alts"]) * 100 <= n_slots, (geometry, mode, seed)
            inserted = set().union(*(d.keys() for d in dumps))
            assert 100 <= sum(x not in inserted for x in p["sample"]) <= 300
            assert len(p["slot_ids"]) == n_slots and 0 < sum(x in inserted for x in p["slot_ids"]) < n_slots


# ---- the comparator can fail -----------------------------------------------------------------------------------------------------------------
def test_the_comparator_reports_a_count_an_absence_and_an_extra_entry(O):
    a, _ = two_models(O, "k31m11b11", "wrap")
    got = a.dump()
    assert diff_entries(got, a) is None
    assert diff_entries(tuple(x[::-1] for x in got), a) is None  # the order of an enumeration is not compared
    off = tuple(x.copy() for x in got)
    off[3][17] += 1
    msg = diff_entries(off, a)
    assert msg and "1 not in the model" in msg and "1 not in the index" in msg
    assert "0 not in the model" in diff_entries(tuple(x[1:] for x in got), a) and "1 not in the index" in diff_entries(tuple(x[1:] for x in got), a)
    extra = tuple(np.concatenate([x, x[:1]]) for x in got)
    extra[0][-1] ^= np.uint64(4)
    assert "1 not in the model" in diff_entries(extra, a) and "0 not in the index" in diff_entries(extra, a)
    assert diff_entries(tuple(np.concatenate([x, x[:1]]) for x in got), a)  # an identity twice is not the model's index either


@pytest.mark.parametrize("mode", MODES)
def test_the_wrong_modes_model_fails(O, mode):
    geometry = "k63m21b14"
    case, dumps = _case(geometry, mode, SEEDS[geometry, mode][0])
    i, h, right, wrong = sequence_facts(O, case, dumps)["first_divergence"]
    assert diff_entries(right.dump(), right) is None
    assert diff_entries(right.dump(), wrong), (i, h)
    assert right.digest(O) != wrong.digest(O) and not np.array_equal(right.spectrum(), wrong.spectrum())


# ---- the replay itself, on a stand-in for the device ----------------------------------------------------------------------------------------
class FakeHip:
    """The calls op_sequence_worker.replay makes, answered by an IndexModel and the oracle: what a correct library would answer.
    `fault` plants one wrong behaviour."""
    O, fault, files = None, None, {}

    def __init__(self, k, m, b, count_mode="wrap", immediate_inserts=False, part_bits=0):
        self.kmb, self.count_mode, self.model, self.h = (k, m, b), count_mode, IndexModel(count_mode), None
        self.layout = dict(part_bits=part_bits or 24, ext_bits=0)
        self.ref = self.O.index_new(k, m, b)
        self.L = self

    def close(self):
        self.O.index_free(self.ref)

    def insert_reads(self, reads):
        self.model.insert(batch_dump(self.O, reads, *self.kmb))

    def prune(self, lo, hi):
        return self.model.prune(lo, hi)

    def merge(self, other):
        n = self.model.merge(other.model)
        if self.fault == "merge touches other" and other.model.d:
            other.model.d.pop(next(iter(other.model.d)))
        return n

    def subtract(self, other):
        return self.model.subtract(other.model)

    def intersect(self, other, count="left"):
        return self.model.intersect(other.model, "left" if self.fault == "intersect ignores the rule" else count)

    def filter_joint(self, other, *w, keep_absent=False):
        return self.model.filter_joint(other.model, w + (keep_absent,)) + (self.fault == "filter_joint miscounts")

    def save(self, path):
        self.files[path] = (self.model.save(), self.count_mode, self.kmb, self.layout)
        open(path, "w").close()
        return len(self.model.d)

    def clear(self):
        self.model.clear()

    def load(self, path, room=False):
        return self.model.load(self.files[path][0])

    @classmethod
    def open(cls, path, room=False, immediate_inserts=False):
        snap, mode, kmb, layout = cls.files[path]
        ix = cls(*kmb, count_mode=mode)
        ix.layout = layout
        ix.load(path)
        return ix

    def stats(self):
        n, nb = self.model.stats(self.O, self.ref) if self.model.d else (0, 0)
        return dict(nb_kmers=n, nb_buckets=nb, largest_bucket=len(self.model.d))

    def checksum(self):
        return self.model.digest(self.O)

    def count_spectrum(self):
        return self.model.spectrum()

    def enumerate(self, min_count=0, max_count=255):
        return self.model.dump(min_count, max_count)

    def lookup(self, lo, hi, idx):
        d = self.model.d
        keys = list(zip(hi.tolist(), lo.tolist(), idx.tolist()))
        found = np.array([x in d for x in keys], np.uint8)
        if self.fault == "lookup finds a removed entry" and not found.all():
            found[int(np.argmin(found))] = 1
        return np.array([d.get(x, 0) for x in keys], np.uint8), found

    def get_kmers(self, reads):
        from index_model import expected_slots, slot_identities
        ids, base, alts = slot_identities(self.O, reads, self.kmb[0], self.kmb[1])
        want, _ = expected_slots(self.model, ids, alts)
        return (want & 0xff).astype(np.uint8), (want & 0x100) != 0, base

    def compare(self, other):
        return self.model.compare(other.model)

    def joint_spectrum(self, other):
        return self.model.joint_spectrum(other.model)

    def brisk_hip_enumerate(self, h, cursor, lo, hi, idx, cnt, cap, n_out):
        d = self.model.dump()
        n = min(cap, len(d[0]))
        for out, src in zip((lo, hi, idx, cnt), d):
            out[:n] = src[:n]
        cursor._obj.value, n_out._obj.value = 1, n
        return 0


class FakeModule:
    BriskHip = FakeHip


def test_the_replay_passes_on_a_correct_stand_in_and_names_a_planted_fault(O, tmp_path):
    from op_sequence_worker import SequenceFailure, replay
    FakeHip.O = O
    case = make_case(SEEDS["k63m21b14", "wrap"][1], "k63m21b14", "wrap")
    assert {"merge", "filter_joint"} <= {op["op"] for op in case["ops"]} and any(op.get("rule") in ("min", "max", "sum") for op in case["ops"])
    try:
        FakeHip.fault = None
        assert replay(FakeModule, O, case, str(tmp_path)) > 0
        for fault, word in (("merge touches other", "`other` is not what it was"), ("intersect ignores the rule", "checksum"), ("filter_joint miscounts", "returned"),
                            ("lookup finds a removed entry", "lookup")):
            FakeHip.fault = fault
            with pytest.raises(SequenceFailure) as e:
                replay(FakeModule, O, case, str(tmp_path))
            msg = str(e.value)
            assert word in msg and "seed %d" % case["seed"] in msg and "operations so far" in msg and "operation " in msg, (fault, msg[:300])
        saturating = make_case(SEEDS["k63m21b14", "saturate"][0], "k63m21b14", "saturate")  # the handles count in one mode, the model in the other
        FakeHip.fault = None
        real = FakeHip.__init__

        def wrong_mode(self, k, m, b, count_mode="wrap", **kw):
            real(self, k, m, b, count_mode="wrap", **kw)
            self.count_mode = count_mode
        FakeHip.__init__ = wrong_mode
        try:
            with pytest.raises(SequenceFailure, match="hot"):
                replay(FakeModule, O, saturating, str(tmp_path))
        finally:
            FakeHip.__init__ = real
    finally:
        FakeHip.fault = None
