"""Case builders of the intake tests (test_intake_cpu.py, test_intake.py): no device, no library.  The rule itself is
brisk_amd.fragments_from_reads; what is here builds inputs that reach the kernels' corners, and restates the outputs of
brisk_hip_intake_ascii (packed words, starts) from a fragment table with extract_reference.pack_reads."""
import random

import numpy as np

from extract_reference import pack_reads

VALID = b"ACGTacgt"
INVALID = b"NnRY-\r\n@\x00\x80\xff"


def valid_run(rng, n):
    return bytes(rng.choice(VALID) for _ in range(n))


def invalid_run(rng, n):
    return bytes(rng.choice(INVALID) for _ in range(n))


def fragment_strings(seqs, frags):
    bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
    return [bs[int(f["read"])][int(f["start"]):int(f["start"]) + int(f["len"])] for f in frags]


def expected_outputs(seqs, frags):
    """(packed words with the two zero words, starts uint64[n_fragments + 1]) of a fragment table"""
    return pack_reads(fragment_strings(seqs, frags), 2)


def most_fragments_in_a_word(starts):
    """the largest number of fragments with a nucleotide in one output word"""
    s = np.asarray(starts, np.uint64).astype(np.int64)
    if len(s) < 2:
        return 0
    first, last = s[:-1] // 16, (s[1:] - 1) // 16
    n_words = int(last[-1]) + 1
    hits = np.zeros(n_words + 1, np.int64)
    np.add.at(hits, first, 1)
    np.add.at(hits, last + 1, -1)
    return int(np.cumsum(hits).max())


def crafted_case(L, variant, seed=4242):
    """Reads (bytes) for a handle whose effective minimum is L.  variant 0: the buffer's first byte valid and its last invalid;
    variant 1: the other way round.  Returns (reads, facts): facts names what the case holds, for the test to assert."""
    rng = random.Random(seed + 7 * L + variant)
    buf = bytearray()   # the concatenated bytes
    cuts = [0]          # read boundaries (byte offsets), ascending, may repeat (empty reads)
    facts = {"run_align": set(), "boundary_align": set(), "valid_boundary": 0}

    def boundary():
        cuts.append(len(buf))
        facts["boundary_align"].add(len(buf) % 16)

    for _ in range(3):  # empty reads at the front
        boundary()
    buf += valid_run(rng, 1) if variant == 0 else invalid_run(rng, 1)
    buf += invalid_run(rng, 1)
    # runs of every length 1..40 at every start alignment mod 16
    for length in range(1, 41):
        for align in range(16):
            buf += invalid_run(rng, 1)
            while len(buf) % 16 != align:
                buf += invalid_run(rng, 1)
            facts["run_align"].add((length, len(buf) % 16))
            buf += valid_run(rng, length)
            if rng.random() < 0.15:
                buf += invalid_run(rng, 1)
                boundary()
    buf += invalid_run(rng, 1)
    boundary()
    # read boundaries at every alignment mod 16 between two valid bytes: halves of L and L, L - 1 and L, L and L - 1
    for align in range(16):
        for a, b in ((L, L), (L - 1, L), (L, L - 1), (1, 1)):
            buf += invalid_run(rng, 1)
            while (len(buf) + a) % 16 != align:
                buf += invalid_run(rng, 1)
            buf += valid_run(rng, a)
            boundary()
            facts["valid_boundary"] += 1
            buf += valid_run(rng, b)
    buf += invalid_run(rng, 2)
    boundary()
    for _ in range(5):  # a run of empty reads
        boundary()
    for _ in range(6):  # one-byte reads, valid and not
        buf += valid_run(rng, 1) if rng.random() < 0.5 else invalid_run(rng, 1)
        boundary()
    # fragments of exactly L, one invalid byte apart: several to an output word when L is small
    for _ in range(12):
        buf += valid_run(rng, L) + invalid_run(rng, 1)
    boundary()
    # whole reads that are one fragment, back to back with no invalid byte between
    for _ in range(6):
        buf += valid_run(rng, L + rng.randint(0, 3))
        boundary()
    while len(buf) % 16 in (0, 15):
        buf += invalid_run(rng, 1)
    buf += invalid_run(rng, 1) if variant == 0 else valid_run(rng, 1)
    boundary()
    for _ in range(2):  # empty reads at the end
        boundary()
    reads = [bytes(buf[cuts[i]:cuts[i + 1]]) for i in range(len(cuts) - 1)]
    facts["total"] = len(buf)
    facts["first_valid"] = buf[0] in VALID
    facts["last_valid"] = buf[-1] in VALID
    return reads, facts


def long_cases(L, block):
    """name -> reads: runs that cross many blocks of `block` bytes (the buffer starts on a block boundary when it is 16-byte aligned)"""
    rng = random.Random(99 + L)
    n = 3 * block + 17
    long = valid_run(rng, n)
    cases = {"one_run": [long]}
    for name, at in (("n_at_0", 0), ("n_before_block", block - 1), ("n_on_block", block), ("n_at_last", n - 1)):
        b = bytearray(long)
        b[at] = ord("N")
        cases[name] = [bytes(b)]
    cases["boundary_on_block"] = [valid_run(rng, block), valid_run(rng, 100)]
    far = valid_run(rng, 40 * block)
    cases["short_after_40_blocks"] = [far + b"N" + valid_run(rng, L - 1)]
    cases["short_read_after_40_blocks"] = [far, valid_run(rng, L - 1)]
    cases["exact_read_after_40_blocks"] = [far + valid_run(rng, 5), valid_run(rng, L)]
    return cases


def quality_case(n_reads, seed, n_rate=0.01, read_len=150):
    """error-bearing reads: random bases with `n_rate` N, and random qualities (Phred+33, 2..41)"""
    rng = np.random.default_rng(seed)
    seqs, quals = [], []
    for _ in range(n_reads):
        n = int(rng.integers(read_len // 2, read_len + 1))
        s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
        s[rng.random(n) < n_rate] = ord("N")
        q = (33 + np.minimum(41, np.maximum(2, rng.normal(32, 9, n).astype(np.int64)))).astype(np.uint8)
        seqs.append(s.tobytes())
        quals.append(q.tobytes())
    return seqs, quals
