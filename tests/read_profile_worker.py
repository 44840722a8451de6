"""Worker of test_read_profile.py: one process per environment (the library reads BRISK_PROFILE_SEG and the kernel-variant
settings once).  The per-read profile of the device against profile_from_slots over get_kmers' slots of the same handle.

    read_profile_worker.py parity     the parity-with-slots case over every geometry
    read_profile_worker.py segments   that, and reads whose solid runs begin and end around the segment boundaries of
                                      BRISK_PROFILE_SEG (default 4096), and a run that spans three segments

Prints "ok <n checks>"."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # before the library: torch's HIP runtime first, as in the test process

import brisk_amd
from test_gpu_parity import SPECIAL, _random_reads
from test_kmer_query import GEOMETRIES, packed_on_device, query_set

SOLID_MINS = (0, 1, 2, 3, 255, 256)
COMP = str.maketrans("ACGT", "CATG")  # a substitution: never the same nucleotide


def parity_reads(rng):
    base = _random_reads(rng, 1100, 20_000)
    return base + base[:300] + base[:100] * 2 + SPECIAL + ["A" * 150] * 5 + ["ACGT" * 40] * 3  # counts of 1, 2 and more


def profile_packed(ix, seqs, solid_min):
    d_packed, d_starts, _ = packed_on_device(ix, seqs)
    d_out = torch.full((max(len(seqs), 1) * 32,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ix.read_profile_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), d_out.data_ptr(), solid_min)
    return d_out.cpu().numpy().view(brisk_amd.READ_PROFILE_DTYPE)[:len(seqs)]


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for f in want.dtype.names:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (what, f, int(bad[0]), got[bad[0]], want[bad[0]], len(bad))


def check_against_slots(ix, queries, solid_mins, what, packed=True):
    slots = ix.get_kmers(queries)
    for s in solid_mins:
        want = brisk_amd.profile_from_slots(*slots, s)
        assert_same(ix.read_profile(queries, s), want, (what, "read_profile", s))
        if packed:
            assert_same(profile_packed(ix, queries, s), want, (what, "read_profile_packed", s))
    return slots


def substitute(seq, positions):
    s = list(seq)
    for p in positions:
        s[p] = s[p].translate(COMP)
    return "".join(s)


RUN_GEOMETRY = (31, 15, 14)


def expected_solid(n, k, subs):
    """what the construction says: a substituted nucleotide at p makes the slots [p - k + 1, p] absent and leaves the others as
    they are (every k-mer of the genome is in the index, twice).  That holds where a k-mer has one identity whatever read it is
    scanned in, so these constructions use RUN_GEOMETRY: at k <= 32 only equal m-mers inside one k-mer make the identity depend on
    the context, and the random genomes used here have none.  At k > 32 the re-scan sees the low 64 bits of a k-mer only and the
    identity follows the scan's history: a stretch cut from an inserted read is then NOT all present (the parity cases cover
    k = 63; where a run lies among the slots does not depend on k)."""
    solid = [True] * n
    for p in subs:
        for i in range(max(p - k + 1, 0), min(p, n - 1) + 1):
            solid[i] = False
    return solid


def expected_run(n, k, subs):
    """the first of the longest runs of expected_solid's slots"""
    solid = expected_solid(n, k, subs)
    best, cur = (0, 0), 0
    for i in range(n + 1):
        if i < n and solid[i]:
            cur += 1
        else:
            if cur > best[1]:
                best = (i - cur, cur)
            cur = 0
    return best


def boundary_queries(genome, k, seg):
    """(query, substituted positions): reads cut from `genome` whose solid runs end or begin at a segment boundary, one slot before
    it and one slot after it; a run that spans three segments; whole reads of one, two and three segments and a slot more or less"""
    out = []
    n = 3 * seg + 17  # slots: three whole segments and a short fourth
    assert seg >= 2 and len(genome) >= 4 * seg + 11 + k - 1 + 16
    for j, B in enumerate((seg, 2 * seg, 3 * seg)):
        for d in (-1, 0, 1):
            q = genome[3 * j + d + 1:3 * j + d + 1 + n + k - 1]
            if B + d + k - 1 < len(q):
                out.append((q, [B + d + k - 1]))  # the absent stretch starts at slot B + d: a run ends there
            out.append((q, [B + d - 1]))          # the absent stretch ends at slot B + d - 1: a run begins at B + d
            out.append((q, [B + d - 1, min(B + d + seg + k - 1, len(q) - 1)]))  # a run of one segment's length from there
    n = 4 * seg + 11
    q = genome[7:7 + n + k - 1]
    out.append((q, [seg // 2 - 1, 3 * seg + seg // 2 + k - 1]))  # the run [seg / 2, 3.5 seg): three boundaries inside
    out.append((q, [seg // 2 - 1]))                              # and one that runs to the read's end
    for n in (seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 1, 3 * seg - 1, 3 * seg):
        out.append((genome[3:3 + n + k - 1], []))
    return out


def main(mode):
    assert torch.cuda.is_available()
    checks = 0
    for k, m, b in GEOMETRIES:
        rng = random.Random(k * 7 + m + b)
        reads = parity_reads(rng)
        queries = query_set(rng, reads, k)
        with brisk_amd.BriskHip(k, m, b) as ix:
            ix.insert_reads(reads)
            counts, found, _ = check_against_slots(ix, queries, SOLID_MINS, (k, m, b))
            assert found.any() and not found.all() and len(np.unique(counts[found])) >= 3
        checks += 1
    if mode == "segments":
        seg = int(os.environ.get("BRISK_PROFILE_SEG", "4096"))
        k, m, b = RUN_GEOMETRY
        rng = random.Random(seg)
        genome = "".join(rng.choice("ACGT") for _ in range(4 * seg + 400))
        cases = boundary_queries(genome, k, seg)
        queries = [substitute(q, subs) for q, subs in cases]
        with brisk_amd.BriskHip(k, m, b) as ix:
            ix.insert_reads([genome, genome])  # every k-mer twice
            _, found, base = check_against_slots(ix, queries, (1, 2, 3), ("segments", seg))
            got = ix.read_profile(queries, 2)
            for i, (q, subs) in enumerate(cases):
                n = len(q) - k + 1
                assert found[int(base[i]):int(base[i + 1])].tolist() == expected_solid(n, k, subs), ("the construction does not hold", seg, i, subs)
                assert got["n_kmers"][i] == n and got["n_present"][i] == got["n_solid"][i]
                assert (int(got["run_start"][i]), int(got["run_len"][i])) == expected_run(n, k, subs), (seg, i, subs, got[i])
        checks += 1
    print(f"ok {checks}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "parity")
