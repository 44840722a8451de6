"""Worker of tests/test_setops.py, one process per case (SETOPS_WORKER_CASE) so that the library reads its environment afresh and
a case runs under its own time limit.  stdout carries `key value` lines and ends with `ok`; a mismatch prints what differs and
exits 1.

variants: merge under whatever BRISK_INSERT_GENERIC / BRISK_BINS the parent set, four geometries, against the oracle index that
          received both read sets.
density:  two sets of 400 k error-bearing reads of ONE 4 Mbp genome (tests/density_reads.py; the true k-mers are shared, every
          set has its own errors), k63 m21 b14, default partitions.  merge against the digest of the 16-thread oracle index
          holding both sets; subtract, intersect (min) and compare against a numpy join of the two oracle dumps."""
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import brisk_amd
import oracle

THREADS = 16  # the oracle's; not os.cpu_count(): a test host gives a process a share of its cores


def say(key, value):
    print(key, json.dumps(value), flush=True)


def fail(what):
    print("MISMATCH", what, flush=True)
    sys.exit(1)


def variants(O):
    from test_setops import two_samples
    checks = 0
    for (k, m, b), opts in (((63, 21, 14), {}), ((31, 15, 14), {}), ((31, 11, 11), {}), ((47, 13, 8), dict(part_bits=4))):
        reads_a, reads_b = two_samples(7 * k + m, **(dict(glen=40000, n_a=1800, n_b=1200) if opts else {}))
        h = O.index_new(k, m, b)
        O.index_insert_reads(h, *oracle.pack_reads(reads_a + reads_b))
        want = O.index_digest(h), O.index_stats(h)
        O.index_free(h)
        with brisk_amd.BriskHip(k, m, b, **opts) as ix, brisk_amd.BriskHip(k, m, b, **opts) as src:
            ix.insert_reads(reads_a)
            src.insert_reads(reads_b)
            before = ix.stats()["nb_kmers"]
            added = ix.merge(src)
            st = ix.stats()
            got = ix.checksum(), (st["nb_kmers"], st["nb_buckets"])
            if got != want or added != st["nb_kmers"] - before:
                fail(f"merge {(k, m, b)} {opts}: {got} added {added}, oracle {want}")
            checks += 1
    say("checks", checks)


def _fmix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def join(da, db):
    """indices (into da, into db) of the entries whose (hi, lo, idx) is in both dumps; exact.  One sort of a 64-bit mix of the
    identity finds the candidates: a run of two equal mix values, one entry of each dump with equal identities, is a shared
    entry.  Every other run of equal values (different identities that share a mix value) is joined by identity in a dict."""
    mix = lambda d: _fmix(d[0] ^ _fmix(d[1] ^ _fmix(d[2].astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15))))
    na = len(da[0])
    keys = np.concatenate([mix(da), mix(db)])
    order = np.argsort(keys, kind="stable")  # stable: of two equal keys the one of `da` comes first
    sk = keys[order]
    same = sk[1:] == sk[:-1]
    prev = np.concatenate([[False], same])  # equal to the one before
    nxt = np.concatenate([same, [False]])   # equal to the one after
    first = np.nonzero(nxt & ~prev)[0]      # first position of every run of two or more
    pair = ~nxt[first + 1]                  # runs of exactly two
    i0, i1 = order[first[pair]], order[first[pair] + 1]
    ident = lambda i: tuple(np.where(i < na, x[np.minimum(i, na - 1)], y[np.maximum(i, na) - na]) for x, y in zip(da[:3], db[:3]))
    clean = (i0 < na) & (i1 >= na)
    for u, v in zip(ident(i0), ident(i1)):
        clean &= u == v
    ia, ib = [i0[clean]], [i1[clean] - na]
    # what is left: pairs that are not one shared entry, and longer runs
    odd = np.zeros(len(order), bool)
    odd[first[pair][~clean]] = True
    odd[first[~pair]] = True
    rest = []
    for f in np.nonzero(odd)[0]:
        j = f
        while True:
            rest.append(order[j])
            if not nxt[j]:
                break
            j += 1
    rest = np.array(rest, np.int64)
    if len(rest):
        ids = list(zip(*(x.tolist() for x in ident(rest))))
        in_a = {key: int(i) for key, i in zip(ids, rest) if i < na}
        hits = [(in_a[key], int(i) - na) for key, i in zip(ids, rest) if i >= na and key in in_a]
        ia.append(np.array([h[0] for h in hits], np.int64))
        ib.append(np.array([h[1] for h in hits], np.int64))
    ia, ib = np.concatenate(ia), np.concatenate(ib)
    assert all(np.array_equal(x[ia], y[ib]) for x, y in zip(da[:3], db[:3]))
    assert len(np.unique(ia)) == len(ia) and len(np.unique(ib)) == len(ib)
    return ia, ib


def density(O):
    from density_reads import dense_reads, random_genome
    k, m, b = 63, 21, 14
    genome = random_genome(4_000_000, 77)
    gen = dict(repeat_len=1000, repeat_copies=4, n_special=60)
    sets = [dense_reads(400_000, k, 4_000_000, seed, e=0.01, genome=genome, **gen) for seed in (2101, 2102)]
    t0 = time.time()
    hs = []
    for flat, offs in sets:
        h = O.index_new(k, m, b)
        O.index_insert_reads(h, flat, offs, threads=THREADS)
        hs.append(h)
    hab = O.index_new(k, m, b)
    for flat, offs in sets:
        O.index_insert_reads(hab, flat, offs, threads=THREADS)
    da, db = O.index_dump(hs[0]), O.index_dump(hs[1])
    want_merge = O.index_digest(hab), O.index_stats(hab)
    ia, ib = join(da, db)
    say("oracle", dict(seconds=round(time.time() - t0, 1), a=len(da[0]), b=len(db[0]), shared=len(ia), merged=want_merge[1][0]))
    if not (len(ia) * 20 > len(da[0]) and len(ia) < len(da[0]) * 0.9):
        fail("the two sets do not share a part of their entries")
    ca, cb = da[3][ia].astype(np.int64), db[3][ib].astype(np.int64)
    only_a = np.ones(len(da[0]), bool)
    only_a[ia] = False
    want_sub = O.digest_entries(*(x[only_a] for x in da))
    want_int = O.digest_entries(da[0][ia], da[1][ia], da[2][ia], np.minimum(ca, cb).astype(np.uint8))
    want_cmp = dict(both=len(ia), only_self=len(da[0]) - len(ia), only_other=len(db[0]) - len(ib), sum_min=int(np.minimum(ca, cb).sum()), sum_self=int(ca.sum()),
                    sum_other=int(cb.sum()))

    def index(i):
        ix = brisk_amd.BriskHip(k, m, b, immediate_inserts=True)
        ix.insert_flat(*sets[i])
        return ix
    t0 = time.time()
    a, bb = index(0), index(1)
    cs_b = bb.checksum()
    if (a.checksum(), cs_b) != (O.index_digest(hs[0]), O.index_digest(hs[1])):
        fail("the indexes differ from the oracle's before any operation")
    times = {}

    def timed(name, f):
        t = time.time()
        out = f()
        times[name] = round(time.time() - t, 4)
        return out
    got = timed("compare", lambda: a.compare(bb))
    if got != want_cmp:
        fail(f"compare {got}, numpy {want_cmp}")
    added = timed("merge", lambda: a.merge(bb))
    st = a.stats()
    if (a.checksum(), (st["nb_kmers"], st["nb_buckets"])) != want_merge or added != len(db[0]) - len(ib):
        fail(f"merge: {a.checksum()} {st} added {added}, oracle {want_merge}")
    a.close()
    a = index(0)
    removed = timed("subtract", lambda: a.subtract(bb))
    if removed != len(ia) or a.checksum() != want_sub:
        fail(f"subtract removed {removed} checksum {a.checksum()}, numpy {len(ia)} {want_sub}")
    a.close()
    a = index(0)
    removed = timed("intersect_min", lambda: a.intersect(bb, count="min"))
    if removed != len(da[0]) - len(ia) or a.checksum() != want_int:
        fail(f"intersect removed {removed} checksum {a.checksum()}, numpy {len(da[0]) - len(ia)} {want_int}")
    if bb.checksum() != cs_b:
        fail("src changed")
    a.close()
    bb.close()
    say("device", dict(seconds=round(time.time() - t0, 1), calls_s=times))
    for h in hs + [hab]:
        O.index_free(h)


if __name__ == "__main__":
    oracle.build(ref=False)
    {"variants": variants, "density": density}[os.environ.get("SETOPS_WORKER_CASE", "variants")](oracle.Oracle())
    print("ok", flush=True)
