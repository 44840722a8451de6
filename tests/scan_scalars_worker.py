"""Worker of tests/test_scan_scalars.py: one process per environment (the library reads BRISK_SCAN_QCAP when a handle is created, and
the test wants the whole process under one setting).  `python scan_scalars_worker.py`; results go to stdout as `NAME <json>` lines,
the last line is `ok` (the conventions of tests/insert_pair_worker.py).  Every index is compared with the oracle's index of the same
reads here: entries, buckets, the sum of the counts, the full enumeration and the digest; every query with the oracle's answers."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

import oracle
from density_reads import _LETTERS, as_strings, random_genome, substitute

M, B = 21, 14
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def out(name, value):
    print(name, json.dumps(value), flush=True)


def reads_of(lens, seed, e=0.01):
    """Reads of the given lengths cut from a random genome at random places, every second one from the other strand, then substitutions at
    rate e (tests/density_reads.py: substitute).  (flat, offs) as the C-ABI and the oracle take them."""
    rng = np.random.default_rng([seed, 0x5ca1])
    glen = max(4000, 10 * int(max(lens)))
    g = _LETTERS[random_genome(glen, seed)].tobytes()
    seqs = []
    for i, L in enumerate(lens):
        at = int(rng.integers(0, glen - L + 1))
        s = g[at:at + L]
        seqs.append(s.translate(COMP)[::-1] if i & 1 else s)
    flat, offs = oracle.pack_reads(seqs)
    return (substitute(flat, e, seed) if e > 0 else flat), offs


def mixed_lengths(k):
    """Three waves of one block.  Wave 0 cycles through the lengths at which the step loop does something else: k - 1 (no k-mer: a dead lane
    beside live ones), k, k + 1, k + 30 .. k + 33 (31 .. 34 steps: the 32-step buffer reload is not taken, taken for one step, for two)
    and 150.  Wave 1: the trip count comes from a single lane (one read of 150 among reads of at most two k-mers).  Wave 2: no lane has a
    k-mer, the wave goes straight to the final flush while the block's other waves work."""
    cycle = [k - 1, k, k + 1, k + 30, k + 31, k + 32, k + 33, 150]
    wave0 = [cycle[i % 8] for i in range(64)]
    wave1 = [k - 1, k, k + 1] * 21 + [k]
    wave1[37] = 150
    wave2 = [k - 1] * 40 + [k - 2] * 24
    return wave0 + wave1 + wave2


SHAPES = {
    # name: (k, lengths, seed)
    "mixed": lambda: (63, mixed_lengths(63), 11),
    # 1094 = 1024 + 64 + 6: not a multiple of 64 nor of 1024; whatever the block size (a multiple of 64 up to 1024), the last block has a
    # wave with six reads and waves with none
    "incomplete-blocks": lambda: (63, [100 + (37 * i) % 51 for i in range(1094)], 12),
    # 400-nt reads with errors: 338 steps and a dozen super-k-mers or more per lane, several flushes of the emit queue inside the step loop
    "dense": lambda: (63, [400] * 1500 + [250] * 36, 13),
    # run-time k and m: the generic body (launch_scan has no instantiation for k = 61)
    "generic": lambda: (61, mixed_lengths(61) + [150] * 300 + [400] * 84, 14),
}


def want_index(O, k, flat, offs):
    h = O.index_new(k, M, B)
    try:
        O.index_insert_reads(h, flat, offs)
        nk, nb = O.index_stats(h)
        lo, hi, idx, cnt = O.index_dump(h)
        return dict(nk=nk, nb=nb, sum=int(np.asarray(cnt, np.uint64).sum()), lines=oracle.multiset_lines(lo, hi, idx, cnt, k),
                    digest=list(O.digest_entries(lo, hi, idx, cnt)))
    finally:
        O.index_free(h)


def insert_and_check(B_, O, name):
    k, lens, seed = SHAPES[name]()
    flat, offs = reads_of(lens, seed)
    want = want_index(O, k, flat, offs)
    with B_.BriskHip(k, M, B, immediate_inserts=True) as ix:
        ix.insert_flat(flat, offs)
        st = ix.stats()
        lo, hi, idx, cnt = ix.enumerate()
        assert (st["nb_kmers"], st["nb_buckets"]) == (want["nk"], want["nb"]), (name, st, want["nk"], want["nb"])
        assert int(np.asarray(cnt, np.uint64).sum()) == want["sum"], name
        assert oracle.multiset_lines(lo, hi, idx, cnt, k) == want["lines"], name
        digest = list(ix.checksum())
        assert digest == want["digest"], (name, digest, want["digest"])
        live = int((np.diff(offs.astype(np.int64)) >= k).sum())
        out(name, {"digest": digest, "entries": st["nb_kmers"], "records": st["nb_skmers"], "reads": len(lens), "live": live})


def queries(B_, O):
    """The query scan (MODE 1) and the per-position scan (MODE 3) over the same reads as the inserts: the mixed wave, the incomplete
    block's tail and dense reads (their flush parameters differ from the insert's: tags, slot bases), against an index of the dense
    reads; a third of the queries are reads the index has never seen."""
    from test_kmer_query import as_u16, assert_slots, expected_all

    k = 63
    flat, offs = reads_of(*SHAPES["dense"]()[1:])
    seen = as_strings(flat, offs)
    q = as_strings(*reads_of(mixed_lengths(k), 11)) + seen[:150] + as_strings(*reads_of([400] * 60 + [150] * 46, 99)) + seen[1400:1500]
    h = O.index_new(k, M, B)
    try:
        O.index_insert_reads(h, flat, offs)
        qf, qo = oracle.pack_reads(q)
        want_sums = O.index_query_reads(h, qf, qo)
        want, alts, base = expected_all(O, h, q, k, M)
    finally:
        O.index_free(h)
    with B_.BriskHip(k, M, B, immediate_inserts=True) as ix:
        ix.insert_flat(flat, offs)
        sums = ix.get_reads(q)
        assert np.asarray(sums, np.uint64).tolist() == np.asarray(want_sums, np.uint64).tolist(), "get_reads"
        counts, found, got_base = ix.get_kmers(q)
        assert np.array_equal(got_base, base)
        assert_slots(as_u16(counts, found), want, alts, "get_kmers")
    out("queries", {"reads": len(q), "slots": int(base[-1]), "found": int(np.asarray(found).sum()), "sum": int(np.asarray(sums, np.uint64).sum())})


if __name__ == "__main__":
    import brisk_amd

    oracle.build(ref=False)
    O_ = oracle.Oracle()
    for name_ in SHAPES:
        insert_and_check(brisk_amd, O_, name_)
    queries(brisk_amd, O_)
    print("ok")
