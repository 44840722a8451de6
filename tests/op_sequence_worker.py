"""Replays the operation sequences of tests/index_model.py on the device, checking the handles against the host model after every
operation.  tests/test_op_sequences.py calls replay() case by case, and starts this file as a child process per kernel variant
(the library reads BRISK_INSERT_GENERIC, BRISK_BINS, BRISK_HUGE_AT, BRISK_DEFER, ... once per process):

    python tests/op_sequence_worker.py                       one seed of each geometry under the environment given; prints "ok <n>"
    python tests/op_sequence_worker.py SEED GEOMETRY MODE    one case, e.g. 3 k47m13b8-pb4 saturate: the way to replay a failure"""
import ctypes as C
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

from index_model import (PRUNE_WINDOWS, TWO_INDEX, WORKER_CASES, IndexModel, apply_op, case_dumps, case_probes, describe, diff_entries, expected_slots,
                         make_case, rows)

PERIOD = 8  # the read-only checks that are not made after every operation: after every eighth, and at the end


class SequenceFailure(AssertionError):
    pass


def replay(B, O, case, tmp_dir):
    """the case on two handles and on the model; raises SequenceFailure at the first difference.  Returns the seconds it took."""
    from test_kmer_query import assert_slots
    t0 = time.time()
    (k, m, b), opts, mode = case["kmb"], case["opts"], case["mode"]
    dumps = case_dumps(O, case)
    probes = case_probes(O, case, dumps)
    models = {h: IndexModel(mode) for h in "AB"}
    h_any = O.index_new(k, m, b)
    ix = {h: B.BriskHip(k, m, b, count_mode=mode, immediate_inserts=case["immediate"][h], **opts) for h in "AB"}
    log = []
    where = "seed %d, %s, %s" % (case["seed"], case["geometry"], mode)

    def fail(i, what):
        raise SequenceFailure("%s: operation %d (%s): %s\noperations so far:\n%s" % (where, i, log[-1] if log else "-", what, "\n".join(log)))

    def check_index(i, h, what):
        """checksum, nb_kmers, nb_buckets, the spectrum and the whole enumeration of handle h against its model"""
        want = models[h].dump()
        cs, st = ix[h].checksum(), ix[h].stats()
        if cs != O.digest_entries(*want):
            fail(i, "%s %s: checksum %s, the model's %s" % (what, h, cs, O.digest_entries(*want)))
        buckets = len(np.unique(O.bucket_ids(h_any, want[0], want[1], want[2]))) if len(want[0]) else 0
        if (st["nb_kmers"], st["nb_buckets"]) != (len(want[0]), buckets):
            fail(i, "%s %s: nb_kmers, nb_buckets %s, the model's %s" % (what, h, (st["nb_kmers"], st["nb_buckets"]), (len(want[0]), buckets)))
        got = ix[h].count_spectrum()
        if not np.array_equal(got, models[h].spectrum()):
            bad = np.nonzero(got != models[h].spectrum())[0]
            fail(i, "%s %s: count_spectrum differs in bins %s" % (what, h, bad[:8].tolist()))
        msg = diff_entries(ix[h].enumerate(), want)
        if msg:
            fail(i, "%s %s: %s" % (what, h, msg))

    def check_lookup(i, h):
        d = models[h].d
        data, found = ix[h].lookup(probes["sample_lo"], probes["sample_hi"], probes["sample_idx"])
        want_found = np.array([x in d for x in probes["sample"]], bool)
        want_data = np.array([d.get(x, 0) for x in probes["sample"]], np.uint8)
        if not np.array_equal(found.astype(bool), want_found):
            j = int(np.nonzero(found.astype(bool) != want_found)[0][0])
            fail(i, "lookup %s: identity %s found %d, in the model %d" % (h, probes["sample"][j], found[j], want_found[j]))
        if not np.array_equal(data[want_found], want_data[want_found]):
            j = int(np.nonzero((data != want_data) & want_found)[0][0])
            fail(i, "lookup %s: identity %s count %d, the model's %d" % (h, probes["sample"][j], data[j], want_data[j]))

    def check_periodic(i):
        lo, hi = PRUNE_WINDOWS[(i // PERIOD) % 4]  # (0, 255) is what every step checks
        for h in "AB":
            msg = diff_entries(ix[h].enumerate(min_count=lo, max_count=hi), models[h].dump(lo, hi))
            if msg:
                fail(i, "enumerate(%d, %d) %s: %s" % (lo, hi, h, msg))
            counts, found, base = ix[h].get_kmers(probes["queries"])
            want, alts = expected_slots(models[h], probes["slot_ids"], probes["alts"])
            if not np.array_equal(base, probes["base"]):
                fail(i, "get_kmers %s: slot bases differ" % h)
            try:
                assert_slots(np.where(found, 0x100 | counts.astype(np.uint16), 0).astype(np.uint16), want, alts, "get_kmers " + h)
            except AssertionError as e:
                fail(i, "get_kmers %s: (what, slot, got, model, slots that differ) = %s" % (h, e))
        got, want = ix["A"].compare(ix["B"]), models["A"].compare(models["B"])
        if got != want:
            fail(i, "A.compare(B) %s, the model's %s" % (got, want))
        got, want = ix["A"].joint_spectrum(ix["B"]), models["A"].joint_spectrum(models["B"])
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            fail(i, "A.joint_spectrum(B) differs: (sa, sb, got, model) %s" % [(int(x), int(y), int(got[x, y]), int(want[x, y])) for x, y in bad[:6]])

    def insert(h, reads, split):
        for j in range(0, len(reads), split or len(reads)):
            ix[h].insert_reads(reads[j:j + (split or len(reads))])

    def device_op(i, op):
        """the operation on the handles; returns what the model's apply_op returns for it"""
        h, name = op["h"], op["op"]
        me = ix[h]
        if name in ("insert", "hot"):
            return insert(h, case["batches"][op["batch"]], op["split"])
        if name == "prune":
            return me.prune(op["lo"], op["hi"])
        if name in TWO_INDEX:
            other = ix[op["other"]]
            if op["pending"] is not None:  # no call on `other` between this insert and the operation: the batch is still deferred
                other.insert_reads(case["batches"][op["pending"]])
            if name == "merge":
                return me.merge(other)
            if name == "subtract":
                return me.subtract(other)
            if name == "intersect":
                return me.intersect(other, count=op["rule"])
            return me.filter_joint(other, *op["window"][:4], keep_absent=op["window"][4])
        if name in ("reload", "reopen"):
            path = os.path.join(tmp_dir, "%s_%d.snap" % (h, i))
            n_saved = me.save(path)
            if name == "reload":
                me.clear()
                n_loaded = me.load(path, room=op["room"])
            else:
                ix[h] = B.BriskHip.open(path, room=op["room"], immediate_inserts=op["immediate"])
                me.close()
                n_loaded = ix[h].stats()["nb_kmers"]
                if ix[h].count_mode != mode or ix[h].layout != me.layout:
                    fail(i, "the handle opened from the snapshot has another layout or count mode")
            os.unlink(path)
            if n_saved != n_loaded:
                fail(i, "%d entries saved, %d loaded" % (n_saved, n_loaded))
            return n_loaded
        if name == "clear":
            return me.clear()
        assert name == "walk"
        return None

    def walk(i, h):
        """a raw brisk_hip_enumerate walk begun and left at a non-zero cursor; nothing else touches the device in this step"""
        if not models[h].d:
            return
        cap = max(ix[h].stats()["largest_bucket"], 1)  # a cap of the largest partition is never refused
        cur, n = C.c_uint64(0), C.c_uint64(0)
        out = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
        rc = ix[h].L.brisk_hip_enumerate(ix[h].h, C.byref(cur), *out, cap, C.byref(n))
        if rc or not n.value or not cur.value:
            fail(i, "the first step of a walk: status %d, %d entries, cursor %d" % (rc, n.value, cur.value))
        part = rows(tuple(x[:n.value] for x in out)).tolist()
        if len(set(part)) != len(part) or not set(part) <= set(rows(models[h].dump()).tolist()):
            fail(i, "the first step of a walk returned entries that are not the model's")

    try:
        for h in "AB":
            if ix[h].layout["part_bits"] != opts.get("part_bits", ix[h].layout["part_bits"]) or (opts.get("part_bits") and ix[h].layout["ext_bits"]):
                fail(-1, "layout %s" % ix[h].layout)
        due = False
        for i, op in enumerate(case["ops"]):
            log.append("%3d %s" % (i, describe(op)))
            want = apply_op(op, models, dumps)
            due |= (i + 1) % PERIOD == 0
            if op["op"] == "walk":
                walk(i, op["h"])
                continue
            got = device_op(i, op)
            if got != want:
                fail(i, "returned %s, the model %s" % (got, want))
            check_index(i, op["h"], "after the operation,")
            if op["op"] in TWO_INDEX:
                check_index(i, op["other"], "`other` is not what it was:")
            check_lookup(i, op["h"])
            if due:
                check_periodic(i)
                due = False
        for h in "AB":
            check_index(len(case["ops"]) - 1, h, "at the end,")
        check_periodic(len(case["ops"]) - 1)
    finally:
        for h in "AB":
            ix[h].close()
        O.index_free(h_any)
    return time.time() - t0


def main(argv):
    import torch

    import brisk_amd
    import oracle
    assert torch.cuda.is_available(), "needs a device"
    oracle.build(ref=False)
    O = oracle.Oracle()
    todo = [(int(argv[0]), argv[1], argv[2])] if argv else WORKER_CASES
    with tempfile.TemporaryDirectory() as tmp:
        for seed, geometry, mode in todo:
            t = replay(brisk_amd, O, make_case(seed, geometry, mode), tmp)
            print("case %d %s %s: %.1f s" % (seed, geometry, mode, t), flush=True)
    print("ok", len(todo))


if __name__ == "__main__":
    main(sys.argv[1:])
