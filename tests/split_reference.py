"""Plain statements of read splitting, for test_split_cpu.py and test_split.py (no device, no library):

* loop_fragments      brisk_hip_solid_runs slot by slot, in plain Python: what fragments_from_slots is checked against;
* slot_cases          crafted slot arrays: every run shape and read size the kernels treat differently;
* gather_reference    brisk_hip_extract_fragments_packed in numpy: the rows of a fragment table gathered nucleotide by nucleotide;
* fragment_case       a fragment table with every alignment of start and length, overlaps, repeats and reads without a row;
* host_slots_model    the slots an index of some reads answers for others, by k-mer hashing in numpy: enough to tell on the CPU
                      whether a read set has reads with two fragments, with none, and short runs."""
import numpy as np

from extract_reference import pack_codes, unpack_codes

FRAGMENT_DTYPE = np.dtype([("read", "<u8"), ("start", "<u4"), ("len", "<u4")])
STATS = ("n_reads", "n_reads_kept", "n_fragments", "n_slots", "n_solid", "n_short", "n_nts_in", "n_nts_out")


def loop_fragments(counts, found, base, k, solid_min, min_len, n_nts_in):
    """([(read, start, len)], stats): one slot at a time"""
    L = max(min_len, k)
    st = dict.fromkeys(STATS, 0)
    st["n_reads"], st["n_slots"], st["n_nts_in"] = len(base) - 1, int(base[-1]), n_nts_in
    rows = []
    for r in range(len(base) - 1):
        run_start, run, kept = 0, 0, False
        n = int(base[r + 1]) - int(base[r])
        for i in range(n + 1):  # (one step past the end closes the open run: a run never crosses into the next read)
            solid = i < n and bool(found[int(base[r]) + i]) and int(counts[int(base[r]) + i]) >= solid_min
            if solid:
                if run == 0:
                    run_start = i
                run += 1
                st["n_solid"] += 1
            elif run:
                if run + k - 1 >= L:
                    rows.append((r, run_start, run + k - 1))
                    st["n_nts_out"] += run + k - 1
                    kept = True
                else:
                    st["n_short"] += run
                run = 0
        st["n_reads_kept"] += kept
    st["n_fragments"] = len(rows)
    return rows, st


def slot_cases(rng, k, n_random=2900, big=True):
    """(counts uint8, found bool, base uint64[n + 1], n_nts_in): about 3000 reads of slots.  Reads of 0, 1, 2, 63, 64, 65, 4095, 4096
    and 4097 slots, all solid, none solid and alternating; a solid last slot next to a solid first slot; present slots of count 0;
    with `big` one read of 3 * 4096 + 5 slots, in front, whose runs end exactly at slot 4095 / 4096 / 4097 of a block of 4096 and 63 / 64 / 65
    of a stretch of 64."""
    reads = []  # (counts, found) per read

    def add(c, f):
        reads.append((np.asarray(c, np.uint8), np.asarray(f, bool)))

    sizes = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097)
    for n in sizes:
        add(np.full(n, 7), np.ones(n, bool))                                   # all solid (the next read begins solid: no run may cross)
        add(np.full(n, 7), np.ones(n, bool))
        add(np.zeros(n), np.zeros(n, bool))                                    # none: absent
        add(np.full(n, 1), np.ones(n, bool))                                   # none at solid_min 2: present but weak
        add(np.where(np.arange(n) % 2 == 0, 9, 0), np.arange(n) % 2 == 0)      # alternating, solid first
        add(np.where(np.arange(n) % 2 == 1, 9, 0), np.arange(n) % 2 == 1)      # alternating, solid last (when n is even)
        add(np.zeros(n), np.ones(n, bool))                                     # present with count 0: solid only at solid_min 0
        c = np.full(n, 3)
        if n:
            c[n // 2] = 0                                                      # one weak slot in the middle: two runs
        add(c, np.ones(n, bool))
    if big:  # the first read: its slot positions are the batch's, so the ends below lie on the kernels' lane, wave and block edges
        n = 3 * 4096 + 5
        c = np.full(n, 5)
        c[[64, 129, 194, 4096, 8193, 12290]] = 0  # runs end at 63, 64 + 64, 65 + 128, and at 4095, 4096 + 4096, 4097 + 8192
        reads.insert(0, (c.astype(np.uint8), np.ones(n, bool)))
    for _ in range(n_random):
        n = rng.choice((0, 0, 1, 2, 3, 5, 20, 38, 70, 88, 120, 188))
        kind = rng.random()
        if kind < 0.15:
            c, f = np.full(n, rng.randint(2, 255)), np.ones(n, bool)
        elif kind < 0.25:
            c, f = np.zeros(n), np.zeros(n, bool)
        else:
            f = np.array([rng.random() < 0.9 for _ in range(n)], bool)
            c = np.array([rng.choice((0, 1, 1, 2, 2, 3, 20, 255)) if rng.random() < 0.2 else 20 for _ in range(n)])
        add(c, f)
    base = np.zeros(len(reads) + 1, np.uint64)
    base[1:] = np.cumsum([len(c) for c, _ in reads], dtype=np.uint64)
    # a read of n > 0 slots has n + k - 1 nucleotides; one without slots is given any length below k
    n_nts = sum(len(c) + k - 1 if len(c) else i % k for i, (c, _) in enumerate(reads))
    return np.concatenate([c for c, _ in reads]), np.concatenate([f for _, f in reads]), base, n_nts


def read_lengths(base, k):
    """the read lengths slot_cases counted in n_nts_in"""
    slots = (base[1:] - base[:-1]).astype(np.int64)
    return np.where(slots > 0, slots + k - 1, np.arange(len(slots)) % k)


def gather_reference(words, starts, frags):
    """-> (out_words with the two zero words after the last, out_starts uint64[n_frags + 1], n_nts)"""
    starts = np.asarray(starts, np.uint64).astype(np.int64)
    read = np.asarray(frags["read"]).astype(np.int64)
    start = np.asarray(frags["start"]).astype(np.int64)
    lens = np.asarray(frags["len"]).astype(np.int64)
    n_reads = len(starts) - 1
    assert (read < n_reads).all() and (lens > 0).all() and (start + lens <= starts[read + 1] - starts[read]).all()
    codes = unpack_codes(words, int(starts[-1]) if n_reads else 0)
    out_starts = np.zeros(len(lens) + 1, np.uint64)
    out_starts[1:] = np.cumsum(lens, dtype=np.uint64)
    total = int(out_starts[-1])
    first = np.cumsum(lens) - lens
    src = np.repeat(starts[read] + start, lens) + (np.arange(total, dtype=np.int64) - np.repeat(first, lens))
    return pack_codes(codes[src], 2), out_starts, total


def fragment_case(rng):
    """(reads, rows): rows (read, start, len) ordered by read, with all 256 (start % 16, len % 16), lengths 1 to 3, several rows to a
    read (overlapping ones among them), reads without a row, the same row twice in a row, and more nucleotides out than in"""
    reads, rows = [], []

    def read(n):
        reads.append("".join(rng.choice("ACGT") for _ in range(n)))
        return len(reads) - 1

    for _ in range(3):
        read(rng.randint(1, 90))                       # reads without a row, at the front
    for a in range(16):
        for b in range(16):
            start, length = a + 16 * rng.choice((0, 1, 2)), (b or 16) + 16 * rng.choice((0, 0, 1, 3))
            r = read(start + length + rng.randint(0, 25))
            rows.append((r, start, length))
            if rng.random() < 0.3:                      # a second row of the read, overlapping the first
                s2 = start + rng.randint(0, length - 1)
                rows.append((r, s2, rng.randint(1, len(reads[r]) - s2)))
            if rng.random() < 0.2:
                read(rng.randint(1, 60))
    for a in range(16):                                 # the shortest rows at every alignment
        r = read(a + 3 + rng.randint(0, 30))
        for length in (1, 2, 3):
            rows.append((r, a, length))
    r = read(100)                                       # the same read whole, three times in a row: more out than in
    rows += [(r, 0, 100)] * 3
    for _ in range(40):                                 # many short rows to a word
        r = read(rng.randint(5, 40))
        for s in range(0, len(reads[r]) - 4, 3):
            rows.append((r, s, rng.randint(1, 4)))
    for _ in range(200):
        r = read(rng.randint(1, 200))
        if rng.random() < 0.3:
            continue
        s = 0
        while s < len(reads[r]) and rng.random() < 0.8:
            n = rng.randint(1, len(reads[r]) - s)
            rows.append((r, s, n))
            s += max(1, n - rng.randint(0, 8))
    for _ in range(3):
        read(rng.randint(1, 90))                       # and at the end
    return reads, rows


def as_table(rows):
    t = np.zeros(len(rows), FRAGMENT_DTYPE)
    if rows:
        a = np.array(rows, np.int64)
        t["read"], t["start"], t["len"] = a[:, 0], a[:, 1], a[:, 2]
    return t


def _window_hashes(codes, k):
    """a 64-bit hash of every window of k codes (wrapping arithmetic: sum of code[i + j] * B^-j)"""
    B, n = np.uint64(0x9E3779B97F4A7C15), len(codes)
    if n < k:
        return np.zeros(0, np.uint64)
    with np.errstate(over="ignore"):
        binv = np.uint64(pow(int(B), -1, 1 << 64))
        pw_inv = np.cumprod(np.concatenate(([np.uint64(1)], np.full(n - 1, binv, np.uint64))), dtype=np.uint64)
        pw = np.cumprod(np.concatenate(([np.uint64(1)], np.full(n - 1, B, np.uint64))), dtype=np.uint64)
        pre = np.concatenate(([np.uint64(0)], np.cumsum((codes.astype(np.uint64) + np.uint64(1)) * pw_inv, dtype=np.uint64)))
        h = (pre[k:] - pre[:-k]) * pw[:n - k + 1]
        h ^= h >> np.uint64(29)
        return h * np.uint64(0xBF58476D1CE4E5B9)


def host_slots_model(flat, offs, k, n_index):
    """(counts uint8, found bool, base): for every k-mer of every read, how often its canonical form occurs in reads [0, n_index) --
    mod 256, as the wrapping index stores it.  By hashing: good for telling what a read set contains, not for comparing answers."""
    offs = np.asarray(offs, np.uint64).astype(np.int64)
    codes = (np.asarray(flat, np.uint8) >> 1) & 3
    hf = _window_hashes(codes, k)
    hr = _window_hashes((codes ^ 2)[::-1], k)[::-1]  # window i of the forward strand is window n - k - i of the reverse complement
    canon = np.minimum(hf, hr)
    lens = offs[1:] - offs[:-1]
    slots = np.maximum(lens - (k - 1), 0)
    base = np.zeros(len(offs), np.uint64)
    base[1:] = np.cumsum(slots, dtype=np.uint64)
    first = np.cumsum(slots) - slots
    pos = np.repeat(offs[:-1], slots) + (np.arange(int(slots.sum()), dtype=np.int64) - np.repeat(first, slots))  # windows inside one read
    mine = canon[pos]
    indexed = mine[:int(base[n_index])]
    keys, cnt = np.unique(indexed, return_counts=True)
    at = np.searchsorted(keys, mine)
    at[at == len(keys)] = 0
    found = keys[at] == mine if len(keys) else np.zeros(len(mine), bool)
    counts = np.where(found, cnt[at] & 0xff, 0).astype(np.uint8) if len(keys) else np.zeros(len(mine), np.uint8)
    return counts, found, base
