"""Worker of tests/test_spectrum_prune.py::test_working_density_case_b: the reads of case B of tests/density_parity_worker.py
(400 k error-bearing reads of a 4 Mbp genome, k63 m21 b14, part_bits = 20) through count_spectrum and prune(2, 255), against the
16-thread oracle's dump.  stdout carries `key value` lines and ends with `ok`; a mismatch prints what differs and exits 1."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import brisk_amd
import oracle
from density_parity_worker import CASES, THREADS
from density_reads import as_strings, dense_reads, entry_diff, take_reads

E = 0.01
N_SAMPLE = 400


def say(key, value):
    print(key, json.dumps(value), flush=True)


def fail(what, detail=""):
    print("MISMATCH", what, flush=True)
    if detail:
        print(detail, flush=True)
    sys.exit(1)


def main():
    cfg = CASES["B"]
    k, m, b = cfg["kmb"]
    seed = 1000 * (ord("B") - 64) + int(round(E * 10000))  # the seed of density_parity_worker.py for this case and rate
    oracle.build(ref=False)
    O = oracle.Oracle()
    flat, offs = dense_reads(cfg["n"], k, cfg["genome"], seed, e=E, **cfg["gen"])
    n = len(offs) - 1
    t0 = time.time()
    h = O.index_new(k, m, b)
    O.index_insert_reads(h, flat, offs, threads=THREADS)
    dump = O.index_dump(h)
    want_spectrum = np.bincount(dump[3], minlength=256).astype(np.uint64)
    singles = int(want_spectrum[1])
    say("oracle", dict(insert_s=round(time.time() - t0, 1), entries=len(dump[0]), singletons=singles))
    if not 2 * singles > len(dump[0]):  # the point of the input: most entries are sequencing errors
        fail(f"only {singles} of {len(dump[0])} entries are singletons")
    mask = dump[3] >= 2
    left = tuple(a[mask] for a in dump)
    want_digest = O.digest_entries(*left)
    want_buckets = len(np.unique(O.bucket_ids(h, left[0], left[1], left[2], threads=THREADS)))

    with brisk_amd.BriskHip(k, m, b, immediate_inserts=True, **cfg["opts"]) as ix:
        ix.insert_flat(flat, offs)
        t0 = time.time()
        got = ix.count_spectrum()
        say("count_spectrum_s", round(time.time() - t0, 3))
        if not np.array_equal(got, want_spectrum):
            bad = np.nonzero(got != want_spectrum)[0]
            fail(f"spectrum: {len(bad)} bins differ, first {int(bad[0])}: {int(got[bad[0]])} want {int(want_spectrum[bad[0]])}")
        st, cs = ix.stats(), ix.checksum()
        if int(got.sum()) != st["nb_kmers"] or int((got * np.arange(256, dtype=np.uint64)).sum()) != cs[1]:
            fail("spectrum sums disagree with stats / checksum")
        # per-read sums on a sample, before: the oracle's own query (reads whose sum is the plain sum of their k-mers' counts)
        rng = np.random.default_rng(seed + 9)
        pick = np.sort(rng.choice(n, N_SAMPLE, replace=False))
        sf, so = take_reads(flat, offs, pick)
        t0 = time.time()
        removed = ix.prune(2, 255)
        say("prune_s", round(time.time() - t0, 3))
        if removed != singles + int(want_spectrum[0]):
            fail(f"prune removed {removed}, the oracle has {singles} singletons and {int(want_spectrum[0])} entries of count 0")
        st, cs = ix.stats(), ix.checksum()
        say("pruned", dict(checksum=cs, nb_kmers=st["nb_kmers"], nb_buckets=st["nb_buckets"]))
        if cs != want_digest or (st["nb_kmers"], st["nb_buckets"]) != (len(left[0]), want_buckets):
            fail(f"after prune: checksum {cs} stats {(st['nb_kmers'], st['nb_buckets'])}, filtered oracle dump {want_digest} {(len(left[0]), want_buckets)}",
                 entry_diff(ix.enumerate(), left, k))
        if not np.array_equal(ix.count_spectrum(), np.where(np.arange(256) >= 2, want_spectrum, 0).astype(np.uint64)):
            fail("spectrum after prune")
        # per-read sums of the sample against the oracle: its per-k-mer answers (tests/test_kmer_query.py) with the singletons
        # absent, added up per read -- for the reads whose oracle sum is the plain sum of their k-mers' counts (no stop at a
        # zero minimizer) and that hold no span that reads the same on both strands
        from test_kmer_query import expected_all
        strings = [s.upper() for s in as_strings(sf, so)]
        want_s, alts, base = expected_all(O, h, strings, k, m)
        full = O.index_query_reads(h, sf, so, threads=THREADS)
        cnt = (want_s & 0xff).astype(np.int64) * ((want_s & 0x100) != 0)
        ambiguous = np.zeros(len(want_s), bool)
        for s0, e0, _ in alts:
            ambiguous[s0:e0] = True
        seg = lambda v: np.array([int(v[int(base[r]):int(base[r + 1])].sum()) for r in range(len(strings))], np.uint64)
        usable = (seg(cnt) == full) & (seg(ambiguous.astype(np.int64)) == 0)
        if usable.mean() < 0.9:
            fail(f"only {int(usable.sum())} of {len(usable)} sampled reads are usable")
        want_sums = seg(np.where(cnt >= 2, cnt, 0))
        got_sums = np.zeros(len(so) - 1, np.uint64)
        ix._chk(ix.L.brisk_hip_get_reads(ix.h, sf, so, len(so) - 1, got_sums))
        if not np.array_equal(got_sums[usable], want_sums[usable]):
            bad = np.nonzero((got_sums != want_sums) & usable)[0]
            fail(f"get_reads after prune: {len(bad)} reads differ, first {int(bad[0])}: {int(got_sums[bad[0]])} want {int(want_sums[bad[0]])}")
        say("read_sample", dict(reads=len(pick), usable=int(usable.sum()), total=int(want_sums[usable].sum())))
    O.index_free(h)
    print("ok", flush=True)


if __name__ == "__main__":
    main()
