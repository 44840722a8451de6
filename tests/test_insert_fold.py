"""The containment fold of k_insert_fast / k_insert_big (DESIGN.md section 4 finding 15): records contained in other records of
their chunk are not expanded, their multiplicities are added over their head's instance slots.  Exact whatever the data, so
the reads here are built to hit its edges, and the index must equal the oracle's -- and the run-time-geometry body's, which
does not fold (BRISK_INSERT_GENERIC=1, in a process of its own: the library reads the variable once)."""
import hashlib
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import oracle

pytestmark = pytest.mark.gpu

CONFIGS = ((63, 21, 14), (31, 15, 14), (31, 11, 11))
_RC = str.maketrans("ACGT", "TGCA")


def _rc(s):
    return s.translate(_RC)[::-1]


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def cases():
    """(name, reads, batches) -- every case is small enough for the oracle."""
    rng = random.Random(1505)
    out = []
    # one long read and its sub-reads at every offset, on both strands: nested records, records that overlap without nesting
    # (a read end cuts a super-k-mer on either side), hundreds of records per partition (several chunks)
    g = _rand(rng, 420)
    subs = [g]
    for L in (64, 90, 150):
        for o in range(0, len(g) - L + 1, 1 if L == 150 else 3):
            subs += [g[o:o + L], _rc(g[o:o + L])]
    out.append(("sub-reads", subs, 2))
    # equal ranges that differ in one base: one-base mutants at every position of a read, a few copies of each (a change
    # inside the minimizer's bucket nucleotides leaves the compacted string alone and moves the routing id)
    g = _rand(rng, 150)
    muts = [g] * 3
    for i in range(len(g)):
        c = rng.choice([x for x in "ACGT" if x != g[i]])
        mu = g[:i] + c + g[i + 1:]
        muts += [mu, mu[20:], _rc(mu)[: 100]]
    out.append(("mutants", muts, 1))
    # the same minimizer-sized core at two loci with different flanks, with sub-reads of both; repeats that put one
    # minimizer at many loci of a read
    two = []
    for _ in range(12):
        core = _rand(rng, 25)
        for _loc in range(2):
            s = _rand(rng, 70) + core + _rand(rng, 70)
            two += [s, s[10:], s[:-15], _rc(s)[5:]]
    two += ["ACGT" * 40, "AACCGGTT" * 20, "A" * 150, "AC" * 75] * 3
    out.append(("two-loci", two, 1))
    # 300+ copies of one locus' sub-reads: counts wrap mod 256
    g = _rand(rng, 200)
    wrap = []
    for o in range(0, 101):
        wrap += [g[o:o + 100]] * 2 + [_rc(g[o:o + 100])]
    out.append(("wrap", wrap, 3))
    return out


def run_cases(brisk_amd, O):
    """Every case under every configuration against the oracle; returns a digest of all the multisets."""
    h = hashlib.sha256()
    for name, reads, batches in cases():
        for k, m, b in CONFIGS:
            want = O.count(reads, k, m, b)
            with brisk_amd.BriskHip(k, m, b) as ix:
                step = (len(reads) + batches - 1) // batches
                for i in range(0, len(reads), step):
                    ix.insert_reads(reads[i:i + step])
                st = ix.stats()
                got = (oracle.multiset_lines(*ix.enumerate(), k), st["nb_kmers"], st["nb_buckets"])
            assert got == want, (name, k, m, b)
            h.update("\n".join(got[0]).encode())
    return h.hexdigest()


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    assert brisk_amd.library_path()
    return brisk_amd


def test_fold_edges_match_the_oracle_and_the_unfolded_body(B, O):
    folded = run_cases(B, O)
    env = dict(os.environ, BRISK_INSERT_GENERIC="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert p.stdout.strip().splitlines()[-1] == "digest " + folded


if __name__ == "__main__":  # the unfolded body's digest, in a process whose library reads BRISK_INSERT_GENERIC
    import brisk_amd

    oracle.build(ref=False)
    print("digest", run_cases(brisk_amd, oracle.Oracle()))
