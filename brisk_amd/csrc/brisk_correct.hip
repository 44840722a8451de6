// brisk_correct.hip -- spectral read correction (brisk_hip_weak_sites / _candidate_windows / _decide_sites / _apply_corrections /
// _correct_*): an isolated substitution leaves one run of weak k-mers whose shape names the nucleotide at fault; the three other bases
// are tried there, and the read is repaired when exactly one of them makes every k-mer of the run solid.  No reference counterpart
// (Quake and BFC repair reads like this before assembly or a second count).  Included by brisk_kernels.hip, behind brisk_split.hip:
// the weak runs are found by the intake's passes over k_split_mask<true>, the candidate windows are gathered by k_extract_gather.
//
// k_split_mask<true>   (brisk_split.hip) the weak mask: the slots of a read that are not solid
// k_correct_class      a weak run {read, first slot i, w slots} -> whole / long / short / site; per block of 256 runs the sites
// k_correct_sites      the sites of the runs, compacted in run order: one vector store a row
// k_correct_site_check a caller's site table: the first bad row flagged
// k_correct_cand_rows  site s -> rows 3s .. 3s + 2 of a fragment table: its window three times (k_split_frag_block / _apply take it)
// CorrectCandPatch     what k_extract_gather calls on a gathered word: candidate c of a site gets the c-th of the three other codes
//                      at the site's position, before the word's one store
// k_correct_cover      per block of 256 sites: their covers (a candidate of a site has `cover` slots)
// k_correct_decide     per site: which of its three candidates have only solid slots -> corrected / ambiguous / unresolved
// k_correct_rows       the correction rows of the corrected sites, compacted in site order: one vector store a row
// k_correct_row_check  a caller's correction table: the first bad row flagged
// k_correct_apply      one lane per word of the stream: the word, with the corrections that fall into it (a search of the table,
//                      which ascends in absolute nucleotide position), stored once

struct CorrectSite {  // brisk_hip_site of include/brisk_hip.h
    u64 read;
    u32 pos, cover;
};
struct CorrectRow {  // brisk_hip_correction of include/brisk_hip.h
    u64 read;
    u32 pos;
    uint8_t from, to;
    uint16_t cover;
};
static_assert(sizeof(CorrectSite) == 16 && sizeof(CorrectRow) == 16, "16-byte rows");

enum { CORRECT_WHOLE = 0, CORRECT_LONG = 1, CORRECT_SHORT = 2, CORRECT_SITE = 3 };
enum { CORRECT_UNRESOLVED = 0, CORRECT_CORRECTED = 1, CORRECT_AMBIGUOUS = 2 };

// the class of the weak run [i, i + w) of a read of n slots; for a site, *pos: the nucleotide that a single substitution must have hit
__device__ __forceinline__ u32 correct_class(u64 i, u64 w, u64 n, u32 k, u32 min_cover, u32* pos) {
    if (i == 0 && i + w == n) return CORRECT_WHOLE;
    if (w > k) return CORRECT_LONG;
    if ((i > 0 && i + w < n && w < k) || w < min_cover) return CORRECT_SHORT;
    *pos = i + w < n ? (u32)(i + w - 1) : (u32)(i + k - 1);
    return CORRECT_SITE;
}
__device__ __forceinline__ u32 correct_run_class(const IntakeFragment& f, const u64* __restrict__ starts, u32 k, u32 min_cover, u32* pos) {
    return correct_class(f.start, f.len, read_slots(starts, f.read, k), k, min_cover, pos);
}

// ctr[0..2] += the block's whole / long / short runs (one atomic a class and block); bsum_sites[block] = its sites
__global__ void __launch_bounds__(256) k_correct_class(const IntakeFragment* __restrict__ runs, u64 n_runs, const u64* __restrict__ starts, u32 k, u32 min_cover,
                                                       u64* __restrict__ bsum_sites, unsigned long long* __restrict__ ctr) {
    __shared__ u64 s[4];
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 cls = ~0u, pos = 0;
    if (j < n_runs) cls = correct_run_class(runs[j], starts, k, min_cover, &pos);
    const u64 n_site = intake_block_sum(cls == CORRECT_SITE, s);
    if (threadIdx.x == 0) bsum_sites[blockIdx.x] = n_site;
    for (u32 c = 0; c < 3; c++) {
        const u64 n = intake_block_sum(cls == c, s);
        if (threadIdx.x == 0 && n) atomicAdd(&ctr[c], (unsigned long long)n);
    }
}

__device__ __forceinline__ void correct_store16(void* __restrict__ out, u32 a, u32 b, u32 c, u32 d) {
    if (((uintptr_t)out & 15) == 0) {
        *reinterpret_cast<uint4*>(out) = uint4{a, b, c, d};
    } else {  // (a caller's table is aligned as its u64 member asks: 8 bytes)
        reinterpret_cast<uint2*>(out)[0] = uint2{a, b};
        reinterpret_cast<uint2*>(out)[1] = uint2{c, d};
    }
}

// the exclusive prefix of `mine` (0 or 1) over the block's 256 lanes; s: 4 words of LDS
__device__ __forceinline__ u64 correct_block_rank(u64 mine, u64* s) {
    u64 x = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(x, o, 64);
        if ((int)(threadIdx.x & 63) >= o) x += y;
    }
    if ((threadIdx.x & 63) == 63) s[threadIdx.x >> 6] = x;
    __syncthreads();
    u64 before = 0;
    for (u32 j = 0; j < (threadIdx.x >> 6); j++) before += s[j];
    __syncthreads();
    return before + x - mine;
}

// bsum_sites: exclusively scanned.  The rows' reads stay the batch's own (the composed calls add the batch's first read to a correction row)
__global__ void __launch_bounds__(256) k_correct_sites(const IntakeFragment* __restrict__ runs, u64 n_runs, const u64* __restrict__ starts, u32 k, u32 min_cover,
                                                       const u64* __restrict__ bsum_sites, CorrectSite* __restrict__ out) {
    __shared__ u64 s[4];
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 cls = ~0u, pos = 0;
    IntakeFragment f{};
    if (j < n_runs) {
        f = runs[j];
        cls = correct_run_class(f, starts, k, min_cover, &pos);
    }
    const u64 at = bsum_sites[blockIdx.x] + correct_block_rank(cls == CORRECT_SITE, s);
    if (cls == CORRECT_SITE) correct_store16(out + at, (u32)f.read, (u32)(f.read >> 32), pos, f.len);
}

// a site's window begins at nucleotide a of its read and has cover + k - 1 nucleotides
__device__ __forceinline__ u32 correct_window_start(u32 pos, u32 k) { return pos >= k - 1 ? pos - (k - 1) : 0; }
// a row is bad when read >= n_reads, cover is 0 or above k, or pos or the window lies beyond the read
__device__ __forceinline__ bool correct_site_ok(const CorrectSite& t, const u64* __restrict__ starts, u64 n_reads, u32 k) {
    if (t.read >= n_reads || t.cover == 0 || t.cover > k) return false;
    const u64 s0 = starts[t.read], s1 = starts[t.read + 1];
    if (s1 < s0 || t.pos >= s1 - s0) return false;
    return (u64)correct_window_start(t.pos, k) + t.cover + k - 1 <= s1 - s0;
}
// flags[0]: the first bad row (atomicMin; ~0 none)
__global__ void __launch_bounds__(256) k_correct_site_check(const CorrectSite* __restrict__ sites, u64 n_sites, const u64* __restrict__ starts, u64 n_reads, u32 k,
                                                            unsigned long long* __restrict__ flags) {
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j < n_sites && !correct_site_ok(sites[j], starts, n_reads, k)) atomicMin(flags, (unsigned long long)j);
}

__global__ void __launch_bounds__(256) k_correct_cand_rows(const CorrectSite* __restrict__ sites, u64 n_sites, u32 k, IntakeFragment* __restrict__ rows) {
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;  // one lane a row: 3 * n_sites of them
    if (j >= 3 * n_sites) return;
    const CorrectSite t = sites[j / 3];
    split_store_row(rows + j, t.read, correct_window_start(t.pos, k), t.cover + k - 1);
}

// the code of nucleotide p of a packed stream
__device__ __forceinline__ u32 correct_code(const u32* __restrict__ packed, u64 p) { return (packed[p >> 4] >> (30 - 2 * (u32)(p & 15))) & 3u; }
// candidate c (0..2) of a site whose base is `from`: the c-th of the three other codes, ascending
__device__ __forceinline__ u32 correct_cand_code(u32 from, u32 c) { return c + (c >= from); }
// word v with the code of its nucleotide i (0..15) replaced
__device__ __forceinline__ u32 correct_put(u32 v, u32 i, u32 code) {
    const u32 sh = 30 - 2 * i;
    return (v & ~(3u << sh)) | (code << sh);
}

// k_extract_gather's patch for a stream of candidate windows: row j is candidate j % 3 of site j / 3.  Word w has been gathered from
// the reads (row j_first holds its first nucleotide); the rows that put their site's nucleotide into it get the candidate's code there.
struct CorrectCandPatch {
    const CorrectSite* sites;
    u32 k;
    __device__ __forceinline__ u32 operator()(u32 v, u64 w, u64 j_first, const u64* __restrict__ out_starts, u64 n_out) const {
        const u64 p = w * 16;
        for (u64 j = j_first; j < n_out && out_starts[j] < p + 16; j++) {
            const u32 pos = sites[j / 3].pos;
            const u64 q = out_starts[j] + (pos - correct_window_start(pos, k));
            if (q < p || q >= p + 16) continue;
            const u32 i = (u32)(q - p);
            v = correct_put(v, i, correct_cand_code((v >> (30 - 2 * i)) & 3u, (u32)(j % 3)));
        }
        return v;
    }
};

__global__ void __launch_bounds__(256) k_correct_cover(const CorrectSite* __restrict__ sites, u64 n_sites, u64* __restrict__ bsum_cover) {
    __shared__ u64 s[4];
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 t = intake_block_sum(j < n_sites ? sites[j].cover : 0, s);
    if (threadIdx.x == 0) bsum_cover[blockIdx.x] = t;
}

// cand_slots: the slots of the candidate stream (brisk_hip_get_kmers_packed over it): candidate c of site s owns `cover` slots from
// 3 * (the covers of the sites before s) + c * cover on.  bsum_cover: exclusively scanned.  dec[s] = kind | to << 8 | from << 16;
// bsum_corr[block] = the block's corrected sites; ctr[0..2] += its corrected / ambiguous / unresolved ones.  The sites are valid.
__global__ void __launch_bounds__(256) k_correct_decide(const uint16_t* __restrict__ cand_slots, const CorrectSite* __restrict__ sites, u64 n_sites, const u64* __restrict__ bsum_cover,
                                                        const u32* __restrict__ packed, const u64* __restrict__ starts, u32 solid_min, u32* __restrict__ dec,
                                                        u64* __restrict__ bsum_corr, unsigned long long* __restrict__ ctr) {
    __shared__ u64 s[4];
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    CorrectSite t{};
    if (j < n_sites) t = sites[j];
    // the covers before this site: a 0 / 1 rank will not do, so the scan is spelled out over the covers
    u64 x = t.cover;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(x, o, 64);
        if ((int)(threadIdx.x & 63) >= o) x += y;
    }
    if ((threadIdx.x & 63) == 63) s[threadIdx.x >> 6] = x;
    __syncthreads();
    u64 before = bsum_cover[blockIdx.x];
    for (u32 i = 0; i < (threadIdx.x >> 6); i++) before += s[i];
    __syncthreads();
    before += x - t.cover;
    u32 kind = ~0u;
    if (j < n_sites) {
        u32 n_pass = 0, which = 0;
        for (u32 c = 0; c < 3; c++) {
            const uint16_t* sl = cand_slots + 3 * before + (u64)c * t.cover;
            bool pass = true;
            for (u32 i = 0; i < t.cover && pass; i++) pass = split_solid(sl[i], solid_min);
            if (pass) {
                n_pass++;
                which = c;
            }
        }
        const u32 from = correct_code(packed, starts[t.read] + t.pos);
        kind = n_pass == 1 ? CORRECT_CORRECTED : n_pass ? CORRECT_AMBIGUOUS : CORRECT_UNRESOLVED;
        dec[j] = kind | (correct_cand_code(from, which) << 8) | (from << 16);
    }
    for (u32 c = 0; c < 3; c++) {
        const u64 n = intake_block_sum(kind == c, s);
        if (threadIdx.x == 0) {
            if (c == CORRECT_CORRECTED) bsum_corr[blockIdx.x] = n;
            if (n) atomicAdd(&ctr[c == CORRECT_CORRECTED ? 0 : c == CORRECT_AMBIGUOUS ? 1 : 2], (unsigned long long)n);
        }
    }
}

// bsum_corr: exclusively scanned; r0: the batch's first read in the call's numbering
__global__ void __launch_bounds__(256) k_correct_rows(const CorrectSite* __restrict__ sites, const u32* __restrict__ dec, u64 n_sites, const u64* __restrict__ bsum_corr, u64 r0,
                                                      CorrectRow* __restrict__ out) {
    __shared__ u64 s[4];
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    const u32 d = j < n_sites ? dec[j] : 0;
    const bool mine = j < n_sites && (d & 0xffu) == CORRECT_CORRECTED;
    const u64 at = bsum_corr[blockIdx.x] + correct_block_rank(mine, s);
    if (!mine) return;
    const CorrectSite t = sites[j];
    const u64 read = t.read + r0;
    correct_store16(out + at, (u32)read, (u32)(read >> 32), t.pos, ((d >> 16) & 3u) | (((d >> 8) & 3u) << 8) | (t.cover << 16));
}

// a row is bad when it is out of range, when `from` is not the base that is there, when to == from (or no code), or when it does
// not lie behind the row before it in (read, pos).  flags[0]: the first bad row (atomicMin; ~0 none).  The read table ascends.
__global__ void __launch_bounds__(256) k_correct_row_check(const CorrectRow* __restrict__ rows, u64 n_rows, const u32* __restrict__ packed, const u64* __restrict__ starts,
                                                           u64 n_reads, unsigned long long* __restrict__ flags) {
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_rows) return;
    const CorrectRow t = rows[j];
    bool ok = t.read < n_reads && t.from < 4 && t.to < 4 && t.from != t.to;
    if (ok) ok = t.pos < starts[t.read + 1] - starts[t.read];
    if (ok) ok = correct_code(packed, starts[t.read] + t.pos) == t.from;
    if (ok && j) {
        const CorrectRow b = rows[j - 1];
        ok = b.read < t.read || (b.read == t.read && b.pos < t.pos);
    }
    if (!ok) atomicMin(flags, (unsigned long long)j);
}

// The patched copy: words [0, n_words + 2) of the stream (its two readable words included).  The table is valid and ascends, so its
// rows' absolute positions starts[read] + pos ascend: the lane of a word finds the first row at or behind the word's first
// nucleotide and takes the rows that fall into the word.
__global__ void __launch_bounds__(256) k_correct_apply(const u32* __restrict__ packed, const u64* __restrict__ starts, const CorrectRow* __restrict__ rows, u64 n_rows, u64 n_words,
                                                       u32* __restrict__ out) {
    const u64 w = (u64)blockIdx.x * 256 + threadIdx.x;
    if (w >= n_words + 2) return;
    u32 v = packed[w];
    if (w < n_words && n_rows) {
        const u64 p = w * 16;
        u64 lo = 0, hi = n_rows;  // the first row with starts[read] + pos >= p
        while (lo < hi) {
            const u64 mid = lo + (hi - lo) / 2;
            if (starts[rows[mid].read] + rows[mid].pos < p) lo = mid + 1;
            else hi = mid;
        }
        for (; lo < n_rows; lo++) {
            const CorrectRow t = rows[lo];
            const u64 q = starts[t.read] + t.pos;
            if (q >= p + 16) break;
            v = correct_put(v, (u32)(q - p), t.to);
        }
    }
    out[w] = v;
}
