"""Saturating counts (brisk_hip_options.count_mode = BRISK_HIP_COUNTS_SATURATE): what tests/test_saturate.py shares, and the worker
of its kernel-variant test -- one process per environment (the library reads BRISK_INSERT_GENERIC, BRISK_HUGE_AT,
BRISK_INSERT_BIG_AT and BRISK_BINS once).  Prints "digest <sha256 of all multisets>".

The yardstick.  The oracle counts mod 256 (and stays as it is), so true counts come from a read set whose counts cannot reach
256: the set B of test_insert_fold.py's "wrap" case -- one random 200-nt locus, and for every offset 0..100 the 100-nt window
twice plus its reverse complement once, 303 reads.  A k-mer lies in at most 3 (100 - k + 1) of them (210 at k = 31, 114 at
k = 63), so O.count(B, k, m, b) is exact: c per identity.  After B has been inserted t times a saturating index holds the same
identities with min(255, t c), a wrapping one (t c) mod 256."""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

import oracle

CONFIGS = ((63, 21, 14), (31, 15, 14), (31, 11, 11))
TS = (1, 2, 3, 5)
_RC = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(_RC)[::-1]


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def base_reads(seed=2025):
    g = rand_seq(random.Random(seed), 200)
    out = []
    for o in range(0, 101):
        out += [g[o:o + 100]] * 2 + [rc(g[o:o + 100])]
    return out


_yard = {}


def yardstick(O, reads_key, reads, k, m, b):
    """{(kmer string, minimizer_idx): exact count}, nb_buckets of `reads` (computed once per key and left unchanged)"""
    key = (reads_key, k, m, b)
    if key not in _yard:
        lines, nk, nb = O.count(reads, k, m, b)
        c = {}
        for line in lines:
            w = line.split()
            c[(w[0], int(w[1]))] = int(w[2])
        assert len(c) == nk and max(c.values()) <= 3 * (100 - k + 1) < 256, "the oracle's counts must be exact"
        _yard[key] = (c, nb)
    return _yard[key]


def nb_buckets(O, reads_key, reads, k, m, b):
    """nb_buckets of `reads`, whose counts need not be exact"""
    key = ("nb", reads_key, k, m, b)
    if key not in _yard:
        _yard[key] = O.count(reads, k, m, b)[2]
    return _yard[key]


def clamp(x):
    return min(255, x)


def wrap(x):
    return x % 256


def lines_of(counts):
    """{identity: count} -> the sorted "KMER idx count" lines of oracle.multiset_lines"""
    return sorted(f"{km} {idx} {c}" for (km, idx), c in counts.items())


def expected(base, t, rule=clamp):
    return {ident: rule(t * c) for ident, c in base.items()}


def check_index(ix, want, nb, k, what):
    """multiset, nb_kmers, nb_buckets, checksum[0..1] and the spectrum of `ix` against {identity: count}; returns the lines"""
    got = oracle.multiset_lines(*ix.enumerate(), k)
    assert got == lines_of(want), what
    st = ix.stats()
    assert (st["nb_kmers"], st["nb_buckets"]) == (len(want), nb), what
    ck = ix.checksum()
    assert ck[:2] == (len(want), sum(want.values())), what
    spec = ix.count_spectrum()
    assert spec.tolist() == np.bincount(list(want.values()), minlength=256).tolist(), what
    return got


def seven_cuts(reads, seed):
    """the reads shuffled and cut into 7 calls of unequal sizes"""
    rng = random.Random(seed)
    r = list(reads)
    rng.shuffle(r)
    cuts = sorted(rng.sample(range(1, len(r)), 6))
    return [r[a:z] for a, z in zip([0] + cuts, cuts + [len(r)])]


def run_cases(brisk_amd, O):
    """The saturating index over B x t for every configuration and t, as one call and as seven shuffled calls, and one read 300
    times and 300 more: each against the yardstick; returns a digest of all the multisets."""
    h = hashlib.sha256()
    B = base_reads()
    for k, m, b in CONFIGS:
        base, nb = yardstick(O, "B", B, k, m, b)
        for t in TS:
            want = expected(base, t)
            for batches in ([B * t], seven_cuts(B * t, 100 * t + k)):
                with brisk_amd.BriskHip(k, m, b, count_mode="saturate") as ix:
                    for part in batches:
                        ix.insert_reads(part)
                    got = check_index(ix, want, nb, k, (k, m, b, t, len(batches)))
                h.update("\n".join(got).encode())
        one, nb1 = yardstick(O, "one", B[:1], k, m, b)
        with brisk_amd.BriskHip(k, m, b, count_mode="saturate") as ix:
            for _ in range(2):
                ix.insert_reads(B[:1] * 300)
                got = check_index(ix, {ident: 255 for ident in one}, nb1, k, (k, m, b, "one read x 300"))
                h.update("\n".join(got).encode())
    return h.hexdigest()


if __name__ == "__main__":
    import brisk_amd

    oracle.build(ref=False)
    print("digest", run_cases(brisk_amd, oracle.Oracle()))
