// brisk_extract.hip -- reads out of a packed stream (brisk_hip_select_intervals / brisk_hip_extract_packed / brisk_hip_trim_* /
// brisk_hip_unpack_ascii): a profile record becomes a nucleotide interval of its read, and the kept intervals are written, back to
// back at nucleotide granularity, as a new packed stream in the layout the scan takes.  No reference counterpart (khmer's
// trim-low-abund and normalize-by-median act on what brisk_hip_read_profile_* measures).  Included by brisk_kernels.hip.
//
// k_select_intervals   one lane per record: the rule of include/brisk_hip.h (brisk_hip_select_rule) -> {start, len}, len 0 = dropped
// k_extract_block      per block of 4096 reads: kept reads and kept nucleotides (64-bit), an interval that leaves its read and a
//                      read table that does not ascend flagged; k_slot_top (brisk_scan.hip) scans the block sums of both
// k_extract_apply      per kept read, in input order: where it starts in the output (out_starts), where its interval starts in the
//                      source (src_pos), which read it was (out_index)
// k_extract_gather     one lane per output word: the kept read that holds the word's first nucleotide is found in out_starts (one
//                      search over the whole table per block, then a search over the few reads the block's words can reach per
//                      lane), its 32 bits come out of one or two source words by a 64-bit shift, and the lane steps to the next kept
//                      read where one ends inside the word.  Every output word is written once, by one plain store: no atomics.
//                      A source word is loaded only when a kept nucleotide lies in it: nothing past the source's last used word.
// k_unpack_ascii       16 nucleotides of a packed stream, from any nucleotide offset, to 16 bytes of ACTG (the inverse of k_pack_ascii)

struct ReadInterval {  // brisk_hip_read_interval of include/brisk_hip.h (brisk_capi.hip asserts that the two agree)
    u32 start, len;
};

#define SELECT_SOLID_RUN 0u
#define SELECT_MEDIAN 1u
#define SELECT_PRESENT 2u

// min_len: the effective one, max(rule.min_len, k)
__global__ void __launch_bounds__(256) k_select_intervals(const ReadProfile* __restrict__ prof, u64 n_reads, u32 k, u32 kind, u32 min_len, u32 lo, u32 hi,
                                                          ReadInterval* __restrict__ out) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const ReadProfile p = prof[r];
    u64 start = 0, len = 0;
    if (p.n_kmers) {
        if (kind == SELECT_SOLID_RUN) {
            if (p.run_len) {
                start = p.run_start;
                len = (u64)p.run_len + k - 1;
            }
        } else {
            bool keep;
            if (kind == SELECT_MEDIAN) keep = lo <= p.median && p.median <= hi;
            else keep = (u64)lo * p.n_kmers <= 1000ull * p.n_present && 1000ull * p.n_present <= (u64)hi * p.n_kmers;
            if (keep) len = (u64)p.n_kmers + k - 1;
        }
    }
    if (len < min_len || len > 0xffffffffull) start = len = 0;  // (an interval of 2^32 nucleotides or more does not fit the record: dropped)
    ReadInterval iv;
    iv.start = (u32)start;
    iv.len = (u32)len;
    out[r] = iv;
}

#define EXT_ITEMS 16
__device__ __forceinline__ u64 ext_min(u64 a, u64 b) { return a < b ? a : b; }
// flags[0]: the first read whose interval leaves it (atomicMin; ~0 none), flags[1]: starts[] does not ascend somewhere
__global__ void __launch_bounds__(256) k_extract_block(const u64* __restrict__ starts, const ReadInterval* __restrict__ iv, u64 n_reads, u64* __restrict__ bsum_reads,
                                                       u64* __restrict__ bsum_nts, unsigned long long* __restrict__ flags) {
    __shared__ u64 s_r[4], s_n[4];
    const u64 base = (u64)blockIdx.x * 256 * EXT_ITEMS;
    u64 reads = 0, nts = 0;
    for (int i = 0; i < EXT_ITEMS; i++) {
        const u64 r = base + (u64)i * 256 + threadIdx.x;
        if (r >= n_reads) continue;
        const u64 s0 = starts[r], s1 = starts[r + 1];
        const ReadInterval v = iv[r];
        if (s1 < s0) atomicOr(flags + 1, 1ull);
        else if ((u64)v.start + v.len > s1 - s0) atomicMin(flags, (unsigned long long)r);
        else if (v.len) {
            reads++;
            nts += v.len;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        reads += __shfl_down(reads, o, 64);
        nts += __shfl_down(nts, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_r[threadIdx.x >> 6] = reads;
        s_n[threadIdx.x >> 6] = nts;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        bsum_reads[blockIdx.x] = s_r[0] + s_r[1] + s_r[2] + s_r[3];
        bsum_nts[blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    }
}

// bsum_*: exclusively scanned, the totals at [gridDim.x].  Intervals are valid here (the host has read the flags).
__global__ void __launch_bounds__(256) k_extract_apply(const u64* __restrict__ starts, const ReadInterval* __restrict__ iv, u64 n_reads, const u64* __restrict__ bsum_reads,
                                                       const u64* __restrict__ bsum_nts, u64* __restrict__ out_starts, u64* __restrict__ out_index, u64* __restrict__ src_pos) {
    __shared__ u64 s_r[4], s_n[4];
    const u64 base = (u64)blockIdx.x * 256 * EXT_ITEMS + (u64)threadIdx.x * EXT_ITEMS;
    u64 t_reads = 0, t_nts = 0;
    for (int i = 0; i < EXT_ITEMS; i++)
        if (base + i < n_reads) {
            const u32 len = iv[base + i].len;
            t_reads += len != 0;
            t_nts += len;
        }
    u64 xr = t_reads, xn = t_nts;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 yr = __shfl_up(xr, o, 64), yn = __shfl_up(xn, o, 64);
        if ((int)(threadIdx.x & 63) >= o) {
            xr += yr;
            xn += yn;
        }
    }
    if ((threadIdx.x & 63) == 63) {
        s_r[threadIdx.x >> 6] = xr;
        s_n[threadIdx.x >> 6] = xn;
    }
    __syncthreads();
    u64 wr = 0, wn = 0;
    for (u32 j = 0; j < (threadIdx.x >> 6); j++) {
        wr += s_r[j];
        wn += s_n[j];
    }
    u64 j = bsum_reads[blockIdx.x] + wr + xr - t_reads;  // kept reads before this lane's
    u64 at = bsum_nts[blockIdx.x] + wn + xn - t_nts;      // and their nucleotides
    for (int i = 0; i < EXT_ITEMS; i++) {
        const u64 r = base + i;
        if (r >= n_reads) break;
        const ReadInterval v = iv[r];
        if (!v.len) continue;
        out_starts[j] = at;
        src_pos[j] = starts[r] + v.start;
        if (out_index) out_index[j] = r;
        j++;
        at += v.len;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out_starts[bsum_reads[gridDim.x]] = bsum_nts[gridDim.x];
}

// the 16 nucleotides from nucleotide `p` of the stream on, first one in the top bits; only the first `take` (1..16) are asked for:
// the second word is loaded when one of them lies in it, and the bits after them are zero
__device__ __forceinline__ u32 packed_window(const u32* __restrict__ packed, u64 p, u32 take) {
    const u64 w = p >> 4;
    const u32 sh = (u32)(p & 15) * 2;
    u64 x = (u64)packed[w] << 32;
    if (sh + 2 * take > 32) x |= packed[w + 1];
    const u32 v = (u32)((x << sh) >> 32);
    return take == 16 ? v : v & ~(0xffffffffu >> (2 * take));
}

// out_starts[0 .. n_out]: ascending from 0, strictly (a kept read has a nucleotide); n_words = ceil(out_starts[n_out] / 16) > 0; the
// grid covers n_words + 2 words: the two after the last one are zero.  patch(v, w, j, out_starts, n_out) has the last say on word w
// before its one store (j: the row that holds the word's first nucleotide): ExtractNoPatch for a plain gather, brisk_correct.hip's
// CorrectCandPatch for candidate windows.
struct ExtractNoPatch {
    __device__ __forceinline__ u32 operator()(u32 v, u64, u64, const u64*, u64) const { return v; }
};
template <class Patch>
__global__ void __launch_bounds__(256) k_extract_gather(const u32* __restrict__ packed, const u64* __restrict__ out_starts, const u64* __restrict__ src_pos, u64 n_out,
                                                        u64 n_words, u32* __restrict__ out, Patch patch) {
    __shared__ u64 s_j0;
    const u64 w0 = (u64)blockIdx.x * 256;
    if (threadIdx.x == 0 && w0 < n_words) {  // the kept read that holds the block's first nucleotide: the last j with out_starts[j] <= p
        const u64 p = w0 * 16;
        u64 lo = 0, hi = n_out - 1;
        while (lo < hi) {
            const u64 mid = lo + (hi - lo + 1) / 2;
            if (out_starts[mid] <= p) lo = mid;
            else hi = mid - 1;
        }
        s_j0 = lo;
    }
    __syncthreads();
    const u64 w = w0 + threadIdx.x;
    if (w >= n_words + 2) return;
    if (w >= n_words) {
        out[w] = 0;
        return;
    }
    const u64 p = w * 16;
    // 16 * threadIdx.x nucleotides further on lies at most that many kept reads further on
    u64 j = s_j0, hi = ext_min(s_j0 + 16 * (u64)threadIdx.x, n_out - 1);
    while (j < hi) {
        const u64 mid = j + (hi - j + 1) / 2;
        if (out_starts[mid] <= p) j = mid;
        else hi = mid - 1;
    }
    u32 v = 0, filled = 0;
    u64 begin = out_starts[j];
    const u64 j_first = j;
    while (filled < 16 && j < n_out) {
        const u64 end = out_starts[j + 1], q = p + filled;
        const u32 take = (u32)ext_min(16 - filled, end - q);
        v |= packed_window(packed, src_pos[j] + (q - begin), take) >> (2 * filled);
        filled += take;
        if (q + take == end) {
            j++;
            begin = end;
        }
    }
    out[w] = patch(v, w, j_first, out_starts, n_out);
}

// bases[i] = "ACTG"[code of nucleotide first_nt + i], 16 per lane
__global__ void __launch_bounds__(256) k_unpack_ascii(const u32* __restrict__ packed, u64 first_nt, u64 n_nts, uint8_t* __restrict__ bases) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 i0 = g * 16;
    if (i0 >= n_nts) return;
    const u32 take = (u32)ext_min(16, n_nts - i0);
    const u32 v = packed_window(packed, first_nt + i0, take);
    const u32 letters = 0x47544341u;  // 'A' 'C' 'T' 'G', code 0 in the low byte
    u32 q[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        u32 x = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) x |= ((letters >> (8 * ((v >> (30 - 2 * (4 * i + j))) & 3u))) & 0xffu) << (8 * j);
        q[i] = x;
    }
    if (take == 16 && ((uintptr_t)(bases + i0) & 15) == 0) {
        *reinterpret_cast<uint4*>(bases + i0) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
        for (u32 i = 0; i < take; i++) bases[i0 + i] = (uint8_t)(q[i >> 2] >> (8 * (i & 3)));
    }
}
