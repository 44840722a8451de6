"""Plain statements of spectral read correction, for test_correct_cpu.py and test_correct.py (no device, no library):

* loop_sites          brisk_hip_weak_sites slot by slot, in plain Python: what sites_from_slots is checked against;
* weak_cases          crafted slot arrays: every run shape, class and read size the kernels treat differently;
* loop_corrections    brisk_hip_decide_sites candidate by candidate, in plain Python;
* candidate_strings   the three candidates of every site by string slicing;
* windows_reference   brisk_hip_candidate_windows in numpy: the windows gathered three times, the substitution put in;
* patch_reference     brisk_hip_apply_corrections in numpy;
* window_case         a site table whose window starts, lengths and substituted positions cover every offset within a word;
* host_route          the composed calls as a composition of host calls (ix: anything with get_kmers and k)."""
import numpy as np

from extract_reference import SHIFTS, pack_codes, pack_reads, unpack_codes
from split_reference import FRAGMENT_DTYPE, gather_reference

SITE_DTYPE = np.dtype([("read", "<u8"), ("pos", "<u4"), ("cover", "<u4")])
CORRECTION_DTYPE = np.dtype([("read", "<u8"), ("pos", "<u4"), ("from", "u1"), ("to", "u1"), ("cover", "<u2")])
STATS = ("n_reads", "n_slots", "n_weak", "n_runs", "n_sites", "n_skip_whole", "n_skip_long", "n_skip_short", "n_corrected", "n_ambiguous", "n_unresolved")
LETTERS = "ACTG"  # the packed layout's codes 0..3


def code_of(ch):
    return (ord(ch) >> 1) & 3


def loop_sites(counts, found, base, k, solid_min, min_cover):
    """([(read, pos, cover)], stats): one slot at a time"""
    c = min_cover or k
    st = dict.fromkeys(STATS, 0)
    st["n_reads"], st["n_slots"] = len(base) - 1, int(base[-1])
    rows = []
    for r in range(len(base) - 1):
        b, n = int(base[r]), int(base[r + 1]) - int(base[r])
        i, w = 0, 0
        for x in range(n + 1):  # (one step past the end closes the open run: a run never crosses into the next read)
            weak = x < n and not (bool(found[b + x]) and int(counts[b + x]) >= solid_min)
            if weak:
                if w == 0:
                    i = x
                w += 1
                st["n_weak"] += 1
                continue
            if not w:
                continue
            st["n_runs"] += 1
            if i == 0 and i + w == n:
                st["n_skip_whole"] += 1
            elif w > k:
                st["n_skip_long"] += 1
            elif i > 0 and i + w < n and w < k:
                st["n_skip_short"] += 1
            elif w < c:
                st["n_skip_short"] += 1
            else:
                st["n_sites"] += 1
                rows.append((r, i + w - 1 if i + w < n else i + k - 1, w))
            w = 0
    return rows, st


def weak_cases(rng, k, n_random=400):
    """(counts uint8, found bool, base uint64[n + 1]): reads of 0, 1, 2, k - 1, k, 63..65 and 4095..4097 slots -- all weak, all solid,
    alternating, present with count 0 and 1; weak runs of k - 1, k and k + 1 slots in the interior, at each edge and as the whole
    read; a weak last slot next to a weak first slot of the next read; random reads behind them."""
    reads = []

    def add(c):  # a read from its counts: 0 absent, else present with that count (a present slot of count 0: add_found)
        c = np.asarray(c, np.int64)
        reads.append((c.astype(np.uint8), c > 0))

    for n in (0, 1, 2, k - 1, k, 63, 64, 65, 4095, 4096, 4097):
        add(np.zeros(n))                                     # one weak run: the whole read
        add(np.full(n, 7))                                   # no weak slot
        add(np.where(np.arange(n) % 2 == 0, 9, 0))           # alternating: runs of one slot
        add(np.full(n, 1))                                   # present, weak at solid_min 2
        reads.append((np.zeros(n, np.uint8), np.ones(n, bool)))  # present with count 0: solid only at solid_min 0
        for w in (k - 1, k, k + 1):
            if n <= w + 2:
                continue
            for i in (0, 1, (n - w) // 2, n - w - 1, n - w):  # left edge, one slot in, the middle, one slot before the end, right edge
                c = np.full(n, 5)
                c[i:i + w] = 0
                add(c)
        if n > 2:                                            # a weak last slot, then a read with a weak first slot
            c = np.full(n, 5)
            c[-1] = 0
            add(c)
            c = np.full(n, 5)
            c[0] = 0
            add(c)
    for w in (k - 1, k, k + 1):                              # the whole read is one run of w slots
        add(np.zeros(w))
    for _ in range(n_random):
        n = rng.choice((0, 1, 3, 5, 12, 20, 38, 70, 120))
        c = np.full(n, 20)
        for _ in range(rng.choice((0, 1, 1, 2, 3))):
            if n:
                i = rng.randrange(n)
                c[i:i + rng.choice((1, 2, k - 1, k, k, k, k + 1, 2 * k))] = rng.choice((0, 1, 1))
        add(c)
    base = np.zeros(len(reads) + 1, np.uint64)
    base[1:] = np.cumsum([len(c) for c, _ in reads], dtype=np.uint64)
    return np.concatenate([c for c, _ in reads]), np.concatenate([f for _, f in reads]), base


def loop_corrections(cand_counts, cand_found, sites, solid_min, from_codes):
    """([(read, pos, from, to, cover)], (n_corrected, n_ambiguous, n_unresolved)): one candidate at a time"""
    rows, at, amb, unres = [], 0, 0, 0
    for s, (read, pos, cover) in enumerate(sites):
        passing = []
        for c in range(3):
            ok = True
            for x in range(cover):
                ok = ok and bool(cand_found[at]) and int(cand_counts[at]) >= solid_min
                at += 1
            if ok:
                passing.append(c)
        if len(passing) == 1:
            others = [x for x in range(4) if x != from_codes[s]]
            rows.append((read, pos, from_codes[s], others[passing[0]], cover))
        elif passing:
            amb += 1
        else:
            unres += 1
    assert at == len(cand_found)
    return rows, (len(rows), amb, unres)


def as_sites(rows):
    t = np.zeros(len(rows), SITE_DTYPE)
    if len(rows):
        a = np.array(rows, np.int64)
        t["read"], t["pos"], t["cover"] = a[:, 0], a[:, 1], a[:, 2]
    return t


def as_corrections(rows):
    t = np.zeros(len(rows), CORRECTION_DTYPE)
    if len(rows):
        a = np.array(rows, np.int64)
        t["read"], t["pos"], t["from"], t["to"], t["cover"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4]
    return t


def candidate_strings(seqs, sites, k):
    """the 3 * n_sites candidates by string slicing, upper case: window [a, a + cover + k - 1), a = max(0, pos - k + 1), the base at
    pos replaced by each of the three other letters in the order of their codes"""
    out = []
    for t in sites:
        s, pos, cover = seqs[int(t["read"])].upper(), int(t["pos"]), int(t["cover"])
        a = max(0, pos - k + 1)
        assert pos < len(s) and a + cover + k - 1 <= len(s)
        for code in range(4):
            if code != code_of(s[pos]):
                out.append(s[a:pos] + LETTERS[code] + s[pos + 1:a + cover + k - 1])
    return out


def windows_reference(words, starts, sites, k):
    """-> (out_words with the two zero words after the last, out_starts uint64[3 n + 1], n_nts)"""
    t = np.asarray(sites)
    rows = np.zeros(3 * len(t), FRAGMENT_DTYPE)
    a = np.maximum(t["pos"].astype(np.int64) - (k - 1), 0)
    rows["read"], rows["start"], rows["len"] = np.repeat(t["read"], 3), np.repeat(a, 3), np.repeat(t["cover"] + (k - 1), 3)
    out, out_starts, total = gather_reference(words, starts, rows)
    codes = unpack_codes(out, total)
    at = out_starts[:-1].astype(np.int64) + np.repeat(t["pos"].astype(np.int64) - a, 3)
    c = np.tile(np.arange(3), len(t))
    codes[at] = c + (c >= codes[at])
    return pack_codes(codes, 2), out_starts, total


def patch_reference(words, starts, corr):
    """the stream with `to` at nucleotide pos of read `read` for every row; every other bit as it was"""
    out = np.array(words, np.uint32)
    t = np.asarray(corr)
    p = np.asarray(starts, np.uint64).astype(np.int64)[t["read"].astype(np.int64)] + t["pos"].astype(np.int64)
    for q, to in zip(p.tolist(), t["to"].tolist()):
        sh = int(SHIFTS[q % 16])
        out[q // 16] = (int(out[q // 16]) & ~(3 << sh)) | (int(to) << sh)
    return out


def patch_strings(seqs, corr):
    """the reads with every row's letter put in (upper case), and how many rows each read has"""
    out, per_read = [list(s) for s in seqs], [0] * len(seqs)
    for t in corr:
        r, pos = int(t["read"]), int(t["pos"])
        assert code_of(out[r][pos]) == int(t["from"]) != int(t["to"])
        out[r][pos] = LETTERS[int(t["to"])]
        per_read[r] += 1
    return ["".join(s) for s in out], per_read


def window_case(rng, k):
    """(reads, [(read, pos, cover)]): sites whose window start, window length and substituted position take every value mod 16 in
    the output stream's words and in the source's, among them pos = 0 and pos = len - 1, covers 1 .. k, and reads with no site"""
    reads, rows = [], []

    def read(n):
        reads.append("".join(rng.choice("ACGT") for _ in range(n)))
        return len(reads) - 1

    read(rng.randint(1, 40))
    r = read(k)                       # one slot: pos = 0 at the left edge is not a site of any run, but any table is taken
    rows.append((r, 0, 1))
    r = read(k)
    rows.append((r, k - 1, 1))        # pos = len - 1
    for cover in range(1, k + 1):
        for _ in range(6):
            kind = rng.choice(("left", "right", "inner"))
            n = cover + k - 1 + rng.randint(1, 40)
            r = read(n)
            if kind == "left":        # window [0, cover + k - 1), pos = cover - 1
                rows.append((r, cover - 1, cover))
            elif kind == "right":     # the run ends the read: pos = i + k - 1, i = n_slots - cover
                i = (n - k + 1) - cover
                rows.append((r, i + k - 1, cover))
            else:                     # any pos at least k - 1 in, the window inside the read
                pos = rng.randint(k - 1, n - cover)
                rows.append((r, pos, cover))
            if rng.random() < 0.2:
                read(rng.randint(1, 30))
    r = read(3 * k + 40)              # two sites of one read
    rows += [(r, k - 1, k), (r, 2 * k + 5, k)]
    read(5)
    return reads, rows


def host_route(ix, seqs, solid_min, min_cover, sites_from_slots, corrections_from_candidates):
    """get_kmers -> sites_from_slots -> candidate strings -> get_kmers -> corrections_from_candidates -> patched strings:
    (CORRECTION rows, stats, patched strings, corrections per read)"""
    k = ix.k
    sites, st = sites_from_slots(*ix.get_kmers(seqs), k, solid_min, min_cover)
    cands = candidate_strings(seqs, sites, k)
    cc, cf, cbase = ix.get_kmers(cands) if cands else (np.zeros(0, np.uint8), np.zeros(0, bool), np.zeros(1, np.uint64))
    assert (np.diff(cbase.astype(np.int64)) == np.repeat(sites["cover"].astype(np.int64), 3)).all()
    frm = [code_of(seqs[int(t["read"])][int(t["pos"])]) for t in sites]
    corr, cnt = corrections_from_candidates(cc, cf, sites, solid_min, frm)
    st = dict(st, n_corrected=cnt["n_corrected"], n_ambiguous=cnt["n_ambiguous"], n_unresolved=cnt["n_unresolved"])
    assert cnt["n_sites"] == st["n_sites"]
    patched, per_read = patch_strings(seqs, corr)
    return corr, st, patched, per_read
