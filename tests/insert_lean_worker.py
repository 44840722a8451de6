"""Worker of tests/test_insert_lean.py: one process per environment (the library reads BRISK_INSERT_LEAN, BRISK_HUGE_AT, BRISK_BINS
and BRISK_DEBUG_INSERT once).  `python insert_lean_worker.py SCENARIO`; every insert is announced on stderr as
`[lean] stage NAME`, so that the parent can tell which `[brisk_hip] path:` lines belong to it; results go to stdout as
`NAME <json>` lines, the last line is `ok`.  Every index is compared with the oracle's full enumeration here."""
import json
import os
import random
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

import oracle
from density_reads import as_strings, concat_reads, dense_reads
from saturate_worker import base_reads, check_index, yardstick

K, M, B = 63, 21, 14
GENOME = 24000
NI_LEAN = 2  # instance slots per lane of k_insert_first (brisk_insert.hip)


def stage(name):
    sys.stderr.write(f"[lean] stage {name}\n")
    sys.stderr.flush()


def out(name, value):
    print(name, json.dumps(value), flush=True)


def reads_a():
    """8,000 reads of a 24 kb genome (coverage 53) at 0.05 % substitutions, with a repeat family: 5,300 partitions.  The thousand
    or so that hold the genome's own minimizers carry 20 to 60 records each, the rest -- minimizers that an error, a cut or a
    tandem read made -- one or two: 6.9 records on average; 20 partitions hold more than 128 distinct k-mers (so more than
    64 * NI_LEAN instances however their records fold) and 22 more than 64 records."""
    return dense_reads(8000, K, GENOME, 77, e=0.0005, repeat_len=400, repeat_copies=8, n_special=40)


def reads_b():
    """other reads of the same genome: they meet the partitions of reads_a"""
    return dense_reads(3000, K, GENOME, 78, e=0.0005, n_special=10)


def reads_c():
    """A batch the forced binned layout can hold (BRISK_BINS=8: a partition's records beyond 8 go to the overflow area, whose
    regions hold some 30 records each at this size): 3,000 reads without tandem reads, 27 records in a partition at most, 546
    partitions with records beyond their bin."""
    return dense_reads(3000, K, GENOME, 81, e=0.001, n_special=0, ragged_share=0.0)


def sub_reads():
    """One 300-nt locus and its sub-reads at every third offset in three lengths, on both strands: the records of one minimizer
    are distinct sub-ranges of one super-k-mer, far more than 64 of them in a partition."""
    rng = random.Random(1606)
    g = "".join(rng.choice("ACGT") for _ in range(300))
    rc = str.maketrans("ACGT", "TGCA")
    subs = [g]
    for L in (70, 100, 150):
        for o in range(0, len(g) - L + 1, 3 if L != 150 else 1):
            subs += [g[o:o + L], g[o:o + L].translate(rc)[::-1]]
    return oracle.pack_reads(subs)


class Want:
    """the oracle's index of some reads: its lines, nb_kmers, nb_buckets, digest and per-partition numbers"""

    def __init__(self, O, parts):
        flat, offs = concat_reads(parts)
        h = O.index_new(K, M, B)
        try:
            O.index_insert_reads(h, flat, offs)
            self.nk, self.nb = O.index_stats(h)
            lo, hi, idx, cnt = O.index_dump(h)
            self.lines = oracle.multiset_lines(lo, hi, idx, cnt, K)
            self.digest = list(O.digest_entries(lo, hi, idx, cnt))
            # partition = routing id >> 4 = bucket id >> 4 at k63 m21 b14 with 2^24 partitions (asserted against the layout)
            part = O.bucket_ids(h, lo, hi, idx) >> 4
            u, c = np.unique(part, return_counts=True)
            self.n_parts = len(u)
            self.parts_over = int((c > 64 * NI_LEAN).sum())  # distinct k-mers: a lower bound of the instances after the fold
            # records per partition, from the oracle's super-k-mer records of every read
            o = offs.astype(np.int64)
            raw = flat.tobytes()
            rec_parts = []
            for i in range(len(o) - 1):
                if o[i + 1] - o[i] >= K:
                    rec_parts.append(O.records(h, raw[o[i]:o[i + 1]], K, M, B)[1] >> 4)
            ru, rcnt = np.unique(np.concatenate(rec_parts), return_counts=True)
            self.parts_many_records = int((rcnt > 64).sum())
            self.records_per_part = float(rcnt.mean())
        finally:
            O.index_free(h)


def check(ix, want, what):
    got = oracle.multiset_lines(*ix.enumerate(), K)
    st = ix.stats()
    assert (st["nb_kmers"], st["nb_buckets"]) == (want.nk, want.nb), (what, st, want.nk, want.nb)
    assert got == want.lines, what
    ck = list(ix.checksum())
    assert ck == want.digest, (what, ck, want.digest)
    return ck


def new_index(B_, **kw):
    ix = B_.BriskHip(K, M, B, immediate_inserts=True, **kw)
    lay = ix.layout
    assert (lay["part_bits"], lay["ext_bits"], lay["record_words"]) == (24, 0, 4), lay
    return ix


def scenario_main(B_, O):
    A, Bq = reads_a(), reads_b()
    wa, wab = Want(O, [A]), Want(O, [A, Bq])
    out("reads_a", {"partitions": wa.n_parts, "over": wa.parts_over, "many_records": wa.parts_many_records, "records_per_partition": wa.records_per_part})
    with new_index(B_) as ix:
        stage("first")
        ix.insert_flat(*A)
        out("first", check(ix, wa, "first batch"))
        stage("second")
        ix.insert_flat(*Bq)
        check(ix, wab, "second batch")
        ix.clear()
        stage("again")
        ix.insert_flat(*A)
        check(ix, wa, "after clear")
        # the flag is conservative: a loaded snapshot, a merge into an empty index
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "a.brisk")
            ix.save(path)
            with new_index(B_) as ld:
                ld.load(path)
                stage("after-load")
                ld.insert_flat(*Bq)
                check(ld, wab, "insert after load")
        with new_index(B_) as mg:
            stage("merge")
            mg.merge(ix)
            stage("after-merge")
            mg.insert_flat(*Bq)
            check(mg, wab, "insert after merge")
    # a partition of more than 64 records inside a first batch
    S = sub_reads()
    ws = Want(O, [A, S])
    out("sub_reads", {"many_records": ws.parts_many_records})
    with new_index(B_) as ix:
        stage("many-records")
        ix.insert_flat(*concat_reads([A, S]))
        check(ix, ws, "more than 64 records in a partition")
    # saturating counts: one read 300 times (255 for each of its k-mers) among 2,000 reads of a 1 Mb genome (coverage 0.3: their
    # counts are small, so the oracle's -- which wraps -- are exact; and with them the batch stays below the 64 records per
    # partition at which k_insert_big takes it)
    hot = base_reads()[0]
    sparse = as_strings(*dense_reads(2000, K, 1000000, 79, e=0.0, p_n=0.0, n_special=0, lower_share=0.0, ragged_share=0.0))
    lines, _, _ = O.count(sparse, K, M, B)
    want = {(w[0], int(w[1])): int(w[2]) for w in (l.split() for l in lines)}
    assert max(want.values()) < 100
    one, _ = yardstick(O, "one", [hot], K, M, B)
    for ident, c in one.items():
        want[ident] = min(255, want.get(ident, 0) + 300 * c)
    nb = O.count(sparse + [hot], K, M, B)[2]
    with B_.BriskHip(K, M, B, immediate_inserts=True, count_mode="saturate") as ix:
        stage("sat")
        ix.insert_reads(sparse[:1000] + [hot] * 300 + sparse[1000:])
        check_index(ix, want, nb, K, "one read x 300 among sparse reads, saturating")
    # deferred inserts: small calls into a fresh index with default options, completed by a reader
    with B_.BriskHip(K, M, B) as ix:
        flat, offs = A
        o = offs.astype(np.int64)
        stage("deferred-calls")
        for a, z in ((0, 2000), (2000, 4500), (4500, len(o) - 1)):
            ix.insert_flat(np.ascontiguousarray(flat[o[a]:o[z]]), (offs[a:z + 1] - offs[a]).astype(np.uint64))
        stage("deferred-complete")
        check(ix, wa, "deferred inserts")


def scenario_one_batch(B_, O, reads=reads_a):
    """one read set in one immediate call, under whatever environment the parent set"""
    A = reads()
    wa = Want(O, [A])
    with new_index(B_) as ix:
        stage("first")
        ix.insert_flat(*A)
        out("first", check(ix, wa, "first batch"))


if __name__ == "__main__":
    import brisk_amd

    oracle.build(ref=False)
    {"main": scenario_main, "one-batch": scenario_one_batch, "one-batch-c": lambda B_, O: scenario_one_batch(B_, O, reads_c)}[sys.argv[1]](brisk_amd, oracle.Oracle())
    print("ok")
