// brisk_intake.hip -- raw reads onto the packed layout (brisk_hip_intake_ascii / brisk_hip_intake_reads / brisk_hip_insert_raw_reads):
// bytes of any value, with an optional quality string, become fragments -- maximal runs of valid bytes inside one read, at least
// min_len long -- written back to back at nucleotide granularity as a packed stream in the layout the scan takes, with a table that
// says where each came from.  With no quality cut this is clean_dna (counter.cpp:130-169) in bulk; the quality cut is Jellyfish's
// --min-qual-char.  Included by brisk_kernels.hip.
//
// Positions are 64-bit and counted from the 16-byte boundary at or below the first byte (x = byte index - a0), so that a lane's 16
// bases are one aligned vector load; the bytes of the first and last lane that lie outside [lo_x, hi_x) are never loaded.
//
// k_intake_check   the read table: ascending, every read below 2^32 bytes
// k_intake_bounds  per read: its start marked in the lane's mask word
// k_intake_first   per block, one thread each: the first read that starts in or behind it (a search of the table)
// k_intake_mask    per lane of 16 bytes: which are valid (a base, at or above the quality threshold); with the read-start bits it
//                  goes to scratch as one u32, so that the later passes read a quarter of a byte per byte and not the input again.
//                  Per block of INTAKE_BLOCK bytes: the last position at which a run can begin, and the two cut counters
// k_intake_reduce / k_intake_top / k_intake_spread   exclusive running maximum of the blocks' last run begins, in two levels: where
//                  the run that enters a block began
// k_intake_count   per block: fragments that END in it, their nucleotides, the valid bytes of runs that are too short (a run's
//                  length is its end minus the carried begin); k_intake_reduce, k_slot_top (brisk_scan.hip) over the partials and
//                  k_intake_spread scan the block sums
// k_intake_apply   per fragment, in input order: its table row, where it starts in the output, where it starts in the source
// k_intake_kept    reads with a fragment: table rows whose read differs from the row before, per block of rows
// k_intake_gather  one lane per output word: the fragment that holds the word's first nucleotide is found in the starts, its up to 16
//                  source bytes are packed, and the lane steps into the next fragment where one ends inside the word.  Every output
//                  word is written once, by one plain store.

#define INTAKE_BLOCK 4096  // bytes per block: 256 lanes of 16 (BRISK_HIP_INTAKE_BLOCK of include/brisk_hip.h)

struct IntakeFragment {  // brisk_hip_fragment of include/brisk_hip.h (brisk_capi.hip asserts that the two agree)
    u64 read;
    u32 start, len;
};

__global__ void __launch_bounds__(256) k_intake_check(const u64* __restrict__ offsets, u64 n_reads, unsigned long long* __restrict__ flags) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const u64 a = offsets[r], b = offsets[r + 1];
    if (b < a) atomicOr(flags, 1ull);
    else if (b - a > 0xffffffffull) atomicOr(flags, 2ull);
}

// 0x80 in every byte of v that is zero (exact: no carry crosses a byte)
__device__ __forceinline__ u32 intake_zero_bytes(u32 v) { return ~(((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v | 0x7f7f7f7fu); }
// bits 0x80 of four bytes -> the low four bits, byte 0 first
__device__ __forceinline__ u32 intake_nibble(u32 z) { return (((z >> 7) * 0x01020408u) >> 24) & 0xfu; }
// four bytes: which are one of ACGTacgt (0x80 per byte)
__device__ __forceinline__ u32 intake_is_base(u32 w) {
    const u32 u = w | 0x20202020u;
    return (intake_zero_bytes(u ^ 0x61616161u) | intake_zero_bytes(u ^ 0x63636363u) | intake_zero_bytes(u ^ 0x67676767u) | intake_zero_bytes(u ^ 0x74747474u)) & 0x80808080u;
}
// four bytes: which are >= thr as unsigned bytes (0x80 per byte); thr4 = thr in every byte
__device__ __forceinline__ u32 intake_ge_bytes(u32 w, u32 thr4) {
    const u32 d = ((w & 0x7f7f7f7fu) | 0x80808080u) - (thr4 & 0x7f7f7f7fu);  // bit 7: low seven bits of w >= those of thr
    const u32 x = w ^ thr4;                                                    // bit 7: the top bits differ, and then w's decides
    return ((x & w) | (~x & d)) & 0x80808080u;
}

__device__ __forceinline__ u64 intake_max(u64 a, u64 b) { return a > b ? a : b; }

// sum over the block's 256 lanes, valid in thread 0; s: 4 words of LDS (reused by the next call: a barrier ends this one)
__device__ __forceinline__ u64 intake_block_sum(u64 v, u64* s) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    const u64 t = s[0] + s[1] + s[2] + s[3];
    __syncthreads();
    return t;
}

// One thread per entry of the read table: the read's start is marked in the zeroed mask words (an atomic OR on scratch: several
// reads may start in one lane).
__global__ void __launch_bounds__(256) k_intake_bounds(const u64* __restrict__ offsets, u64 n_reads, u64 a0, u64 n_lanes, u32* __restrict__ mask) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    const u64 x = offsets[r] - a0;
    if ((x >> 4) < n_lanes) atomicOr(&mask[x >> 4], 0x10000u << (x & 15));
}
// One THREAD per block of input, b = 0 .. nb: first_read[b] = the first r in [0, n_reads] with offsets[r] - a0 >= b * INTAKE_BLOCK
// (n_reads + 1: none).  A search by one lane of every input block, in front of that block's work, is latency that nothing hides;
// here the searches of 256 blocks run side by side in one thread block, and the time does not depend on how long the reads are.
__global__ void __launch_bounds__(256) k_intake_first(const u64* __restrict__ offsets, u64 n_reads, u64 a0, u64 nb, u64* __restrict__ first_read) {
    const u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > nb) return;
    const u64 x = b * INTAKE_BLOCK;
    u64 lo = 0, hi = n_reads + 1;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (offsets[mid] - a0 < x) lo = mid + 1;
        else hi = mid;
    }
    first_read[b] = lo;
}

// thr: 0 no quality cut (quals is not read), else qual_base + min_qual.  mask[lane]: the read-start bits (<< 16) stand; the valid bits are added.
__global__ void __launch_bounds__(256) k_intake_mask(const uint8_t* __restrict__ bases, const uint8_t* __restrict__ quals, u64 a0, u64 lo_x, u64 hi_x, u32 thr,
                                                     u32* __restrict__ mask, u64* __restrict__ carry, u64* __restrict__ bsum_cut_base, u64* __restrict__ bsum_cut_qual) {
    __shared__ u64 s_sum[4];
    const u64 bs = (u64)blockIdx.x * INTAKE_BLOCK;
    const u64 x0 = bs + (u64)threadIdx.x * 16;
    const uint8_t* pb = bases + (ptrdiff_t)(x0 + a0);
    const uint8_t* pq = quals + (ptrdiff_t)(x0 + a0);
    u32 in_range = 0xffffu;  // which of the lane's 16 positions lie in [lo_x, hi_x)
    u32 wb[4] = {0, 0, 0, 0}, wq[4] = {0, 0, 0, 0};
    if (x0 >= lo_x && x0 + 16 <= hi_x) {
        const uint4 q = *reinterpret_cast<const uint4*>(pb);  // (aligned: x0 + a0 is a multiple of 16 from the buffer's address on)
        wb[0] = q.x; wb[1] = q.y; wb[2] = q.z; wb[3] = q.w;
        if (thr) {
            uint4 t;
            __builtin_memcpy(&t, pq, 16);  // (the qualities' alignment is their own)
            wq[0] = t.x; wq[1] = t.y; wq[2] = t.z; wq[3] = t.w;
        }
    } else {  // the peeled head and tail: byte loads, in range only
        in_range = 0;
        for (int i = 0; i < 16; i++) {
            const u64 x = x0 + i;
            if (x < lo_x || x >= hi_x) continue;
            in_range |= 1u << i;
            wb[i >> 2] |= (u32)pb[i] << (8 * (i & 3));
            if (thr) wq[i >> 2] |= (u32)pq[i] << (8 * (i & 3));
        }
    }
    const u32 thr4 = thr * 0x01010101u;
    u32 is_base = 0, q_ok = 0xffffu;
#pragma unroll
    for (int i = 0; i < 4; i++) is_base |= intake_nibble(intake_is_base(wb[i])) << (4 * i);
    if (thr) {
        q_ok = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) q_ok |= intake_nibble(intake_ge_bytes(wq[i], thr4)) << (4 * i);
    }
    is_base &= in_range;
    const u32 valid = is_base & q_ok;
    const u32 bnd = mask[(u64)blockIdx.x * 256 + threadIdx.x] >> 16;
    mask[(u64)blockIdx.x * 256 + threadIdx.x] = valid | (bnd << 16);

    // where a run can begin: after an invalid byte, or at a read's start
    const u32 cutmask = ((~valid & 0xffffu) << 1) | bnd;
    u64 last = cutmask ? x0 + (31 - __clz(cutmask)) : 0;
    for (int o = 32; o > 0; o >>= 1) last = intake_max(last, __shfl_down(last, o, 64));
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = last;
    __syncthreads();
    if (threadIdx.x == 0) carry[blockIdx.x] = intake_max(intake_max(s_sum[0], s_sum[1]), intake_max(s_sum[2], s_sum[3]));
    __syncthreads();
    const u64 cb = intake_block_sum(__popc(in_range & ~is_base), s_sum);
    const u64 cq = intake_block_sum(__popc(is_base & ~q_ok), s_sum);
    if (threadIdx.x == 0) {
        bsum_cut_base[blockIdx.x] = cb;
        bsum_cut_qual[blockIdx.x] = cq;
    }
}

// carry[i] = max(carry[0 .. i - 1]), 0 for the first: in place, one block
__global__ void __launch_bounds__(1024) k_intake_top(u64* __restrict__ carry, u32 nb) {
    __shared__ u64 s_wave[16];
    __shared__ u64 s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (u32 base = 0; base < nb; base += 1024) {
        const u32 i = base + threadIdx.x;
        const u64 v = i < nb ? carry[i] : 0;
        u64 x = v;  // inclusive maximum within the wave
        for (int o = 1; o < 64; o <<= 1) {
            const u64 y = __shfl_up(x, o, 64);
            if ((int)(threadIdx.x & 63) >= o) x = intake_max(x, y);
        }
        if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = x;
        __syncthreads();
        u64 before = s_carry;  // everything before this lane: earlier rounds, earlier waves, earlier lanes of the wave
        for (u32 j = 0; j < (threadIdx.x >> 6); j++) before = intake_max(before, s_wave[j]);
        const u64 up = __shfl_up(x, 1, 64);
        if (threadIdx.x & 63) before = intake_max(before, up);
        if (i < nb) carry[i] = before;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = intake_max(before, v);
        __syncthreads();
    }
}

// A scan over the per-block values in two levels, so that no single block walks millions of them: k_intake_reduce folds every
// INTAKE_SCAN values into one partial, a single block scans the partials (k_intake_top for a maximum, k_slot_top for a sum: a few
// thousand values at most), and k_intake_spread turns the values into their exclusive prefix in place.  MAX: running maximum, else sum.
#define INTAKE_SCAN 1024
template <bool MAX> __device__ __forceinline__ u64 intake_op(u64 a, u64 b) { return MAX ? intake_max(a, b) : a + b; }
template <bool MAX> __global__ void __launch_bounds__(INTAKE_SCAN) k_intake_reduce(const u64* __restrict__ a, u32 n, u64* __restrict__ part) {
    __shared__ u64 s[INTAKE_SCAN / 64];
    const u64 i = (u64)blockIdx.x * INTAKE_SCAN + threadIdx.x;
    u64 v = i < n ? a[i] : 0;
    for (int o = 32; o > 0; o >>= 1) v = intake_op<MAX>(v, __shfl_down(v, o, 64));
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = s[0];
        for (int j = 1; j < INTAKE_SCAN / 64; j++) t = intake_op<MAX>(t, s[j]);
        part[blockIdx.x] = t;
    }
}
// part: exclusively scanned; for a sum the total stands at part[gridDim.x] and goes to a[n]
template <bool MAX> __global__ void __launch_bounds__(INTAKE_SCAN) k_intake_spread(u64* __restrict__ a, u32 n, const u64* __restrict__ part) {
    __shared__ u64 s[INTAKE_SCAN / 64];
    const u64 i = (u64)blockIdx.x * INTAKE_SCAN + threadIdx.x;
    const u64 v = i < n ? a[i] : 0;
    u64 x = v;  // inclusive within the wave
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(x, o, 64);
        if ((int)(threadIdx.x & 63) >= o) x = intake_op<MAX>(x, y);
    }
    if ((threadIdx.x & 63) == 63) s[threadIdx.x >> 6] = x;
    __syncthreads();
    u64 before = part[blockIdx.x];
    for (u32 j = 0; j < (threadIdx.x >> 6); j++) before = intake_op<MAX>(before, s[j]);
    const u64 up = __shfl_up(x, 1, 64);
    if (threadIdx.x & 63) before = intake_op<MAX>(before, up);
    if (i < n) a[i] = before;
    if (!MAX && blockIdx.x == 0 && threadIdx.x == 0) a[n] = part[gridDim.x];
}

// What the count and the apply pass share: the lane's bits, and where the run that enters the lane began.
struct IntakeLane {
    u64 x0, begin_in;
    u32 ends, cutmask;
};
// every thread of the block calls it (barriers inside); s: 4 words of LDS
__device__ __forceinline__ IntakeLane intake_lane(const u32* __restrict__ mask, u64 n_lanes, const u64* __restrict__ carry, u64* s) {
    IntakeLane ln;
    const u64 lane = (u64)blockIdx.x * 256 + threadIdx.x;
    const u32 w = mask[lane], wn = lane + 1 < n_lanes ? mask[lane + 1] : 0u;
    const u32 valid = w & 0xffffu, bnd = w >> 16;
    const u32 valid_next = (valid >> 1) | ((wn & 1u) << 15), bnd_next = (bnd >> 1) | (((wn >> 16) & 1u) << 15);
    ln.x0 = lane * 16;
    ln.ends = valid & (~valid_next | bnd_next);  // a valid byte followed by an invalid one or by a read's start
    ln.cutmask = ((~valid & 0xffffu) << 1) | bnd;
    const u64 mine = ln.cutmask ? ln.x0 + (31 - __clz(ln.cutmask)) : 0;
    u64 x = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(x, o, 64);
        if ((int)(threadIdx.x & 63) >= o) x = intake_max(x, y);
    }
    if ((threadIdx.x & 63) == 63) s[threadIdx.x >> 6] = x;
    __syncthreads();
    u64 before = carry[blockIdx.x];
    for (u32 j = 0; j < (threadIdx.x >> 6); j++) before = intake_max(before, s[j]);
    const u64 up = __shfl_up(x, 1, 64);
    if (threadIdx.x & 63) before = intake_max(before, up);
    __syncthreads();
    ln.begin_in = before;
    return ln;
}
// the run that ends at bit i of the lane began here
__device__ __forceinline__ u64 intake_run_begin(const IntakeLane& ln, u32 i) {
    const u32 cm = ln.cutmask & ((2u << i) - 1u);
    return cm ? ln.x0 + (31 - __clz(cm)) : ln.begin_in;
}

__global__ void __launch_bounds__(256) k_intake_count(const u32* __restrict__ mask, u64 n_lanes, const u64* __restrict__ carry, u32 min_len, u64* __restrict__ bsum_frag,
                                                      u64* __restrict__ bsum_nts, u64* __restrict__ bsum_short) {
    __shared__ u64 s[4];
    const IntakeLane ln = intake_lane(mask, n_lanes, carry, s);
    u64 frags = 0, nts = 0, shorts = 0;
    for (u32 e = ln.ends; e; e &= e - 1) {
        const u32 i = __ffs(e) - 1;
        const u64 len = ln.x0 + i + 1 - intake_run_begin(ln, i);
        if (len >= min_len) {
            frags++;
            nts += len;
        } else shorts += len;
    }
    const u64 f = intake_block_sum(frags, s), n = intake_block_sum(nts, s), sh = intake_block_sum(shorts, s);
    if (threadIdx.x == 0) {
        bsum_frag[blockIdx.x] = f;
        bsum_nts[blockIdx.x] = n;
        bsum_short[blockIdx.x] = sh;
    }
}

// bsum_*: exclusively scanned, the totals at [gridDim.x]
__global__ void __launch_bounds__(256) k_intake_apply(const u32* __restrict__ mask, u64 n_lanes, const u64* __restrict__ carry, u32 min_len, const u64* __restrict__ bsum_frag,
                                                      const u64* __restrict__ bsum_nts, const u64* __restrict__ offsets, u64 n_reads, u64 a0, const u64* __restrict__ first_read,
                                                      IntakeFragment* __restrict__ frags, u64* __restrict__ out_starts, u64* __restrict__ src_pos) {
    __shared__ u64 s[4];
    __shared__ u64 s_f[4], s_n[4];
    const u64 bs = (u64)blockIdx.x * INTAKE_BLOCK;
    const u64 s_r[2] = {first_read[blockIdx.x], first_read[blockIdx.x + 1]};  // the reads that start inside the block: [s_r[0], s_r[1]) of the table
    const IntakeLane ln = intake_lane(mask, n_lanes, carry, s);
    u64 t_frag = 0, t_nts = 0;
    for (u32 e = ln.ends; e; e &= e - 1) {
        const u32 i = __ffs(e) - 1;
        const u64 len = ln.x0 + i + 1 - intake_run_begin(ln, i);
        if (len >= min_len) {
            t_frag++;
            t_nts += len;
        }
    }
    u64 xf = t_frag, xn = t_nts;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 yf = __shfl_up(xf, o, 64), yn = __shfl_up(xn, o, 64);
        if ((int)(threadIdx.x & 63) >= o) {
            xf += yf;
            xn += yn;
        }
    }
    if ((threadIdx.x & 63) == 63) {
        s_f[threadIdx.x >> 6] = xf;
        s_n[threadIdx.x >> 6] = xn;
    }
    __syncthreads();
    u64 wf = 0, wn = 0;
    for (u32 j = 0; j < (threadIdx.x >> 6); j++) {
        wf += s_f[j];
        wn += s_n[j];
    }
    u64 j = bsum_frag[blockIdx.x] + wf + xf - t_frag;  // fragments before this lane's
    u64 at = bsum_nts[blockIdx.x] + wn + xn - t_nts;    // and their nucleotides
    for (u32 e = ln.ends; e; e &= e - 1) {
        const u32 i = __ffs(e) - 1;
        const u64 begin = intake_run_begin(ln, i), len = ln.x0 + i + 1 - begin;
        if (len < min_len) continue;
        // the read that holds `begin`: the last one that starts at or before it (empty reads start there too).  A run that began inside
        // the block lies in the read that was open at the block's start or in one that starts inside it; else the whole table is searched
        u64 lo = 0, hi = n_reads - 1;
        if (begin >= bs && s_r[1]) {
            hi = ext_min(s_r[1], n_reads) - 1;
            lo = ext_min(s_r[0] ? s_r[0] - 1 : 0, hi);
        }
        while (lo < hi) {
            const u64 mid = lo + (hi - lo + 1) / 2;
            if (offsets[mid] - a0 <= begin) lo = mid;
            else hi = mid - 1;
        }
        IntakeFragment f;
        f.read = lo;
        f.start = (u32)(begin - (offsets[lo] - a0));
        f.len = (u32)len;
        frags[j] = f;
        out_starts[j] = at;
        src_pos[j] = begin + a0;
        j++;
        at += len;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out_starts[bsum_frag[gridDim.x]] = bsum_nts[gridDim.x];
}

__global__ void __launch_bounds__(256) k_intake_kept(const IntakeFragment* __restrict__ frags, u64 n_frags, u64* __restrict__ bsum_kept) {
    __shared__ u64 s[4];
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 first = j < n_frags && (j == 0 || frags[j].read != frags[j - 1].read);
    const u64 t = intake_block_sum(first, s);
    if (threadIdx.x == 0) bsum_kept[blockIdx.x] = t;
}

// the first `take` (1..16) source bytes from byte index p on, packed with the first in the top bits; `end`: no byte at or past it is read
__device__ __forceinline__ u32 intake_window(const uint8_t* __restrict__ bases, u64 p, u32 take, u64 end) {
    const uint8_t* src = bases + (ptrdiff_t)p;
    u32 v = 0;
    if (p + 16 <= end) {
        uint4 q;
        __builtin_memcpy(&q, src, 16);
        const u32 ws[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
#pragma unroll
            for (int j = 0; j < 4; j++) v = (v << 2) | ((ws[i] >> (8 * j + 1)) & 3u);
        }
    } else {
        for (u32 i = 0; i < 16; i++) v = (v << 2) | (i < take ? ((src[i] >> 1) & 3u) : 0u);
    }
    return take == 16 ? v : v & ~(0xffffffffu >> (2 * take));
}

// out_starts[0 .. n_out]: ascending from 0, strictly; n_words = ceil(out_starts[n_out] / 16) > 0; the grid covers n_words + 2 words.
// The starts of the fragments that the block's 256 words touch are staged in LDS (two searches of the table per block), where the
// lanes then search and step.  A fragment has at least INTAKE_MIN_LEN nucleotides (intake_impl refuses a smaller effective minimum;
// create's k - b >= 4 with b >= 1 makes it 5 in practice), so the block's 4096 nucleotides touch at most 4096 / INTAKE_MIN_LEN + 1
// fragments, and one start more ends the last: the stage always holds them.
#define INTAKE_MIN_LEN 4
#define INTAKE_STAGE (256 * 16 / INTAKE_MIN_LEN + 2)
__global__ void __launch_bounds__(256) k_intake_gather(const uint8_t* __restrict__ bases, u64 end, const u64* __restrict__ out_starts, const u64* __restrict__ src_pos, u64 n_out,
                                                       u64 n_words, u32* __restrict__ out) {
    __shared__ u64 s_j[2];
    __shared__ u64 s_st[INTAKE_STAGE];
    const u64 w0 = (u64)blockIdx.x * 256;
    const bool body = w0 < n_words;  // (else: the block holds only the zero words behind the stream)
    if (threadIdx.x < 2 && body) {   // the fragments that hold the block's first and last nucleotide: the last j with out_starts[j] <= p
        const u64 p = threadIdx.x == 0 ? w0 * 16 : ext_min((w0 + 256) * 16, out_starts[n_out]) - 1;
        u64 lo = 0, hi = n_out - 1;
        while (lo < hi) {
            const u64 mid = lo + (hi - lo + 1) / 2;
            if (out_starts[mid] <= p) lo = mid;
            else hi = mid - 1;
        }
        s_j[threadIdx.x] = lo;
    }
    __syncthreads();
    const u64 j0 = body ? s_j[0] : 0, j1 = body ? s_j[1] : 0, n_st = j1 - j0 + 2;  // starts j0 .. j1 + 1
    if (body)
        for (u64 i = threadIdx.x; i < n_st; i += 256) s_st[i] = out_starts[j0 + i];
    __syncthreads();
    const u64 w = w0 + threadIdx.x;
    if (w >= n_words + 2) return;
    if (w >= n_words) {
        out[w] = 0;
        return;
    }
    auto start_of = [&](u64 j) -> u64 { return s_st[j - j0]; };
    const u64 p = w * 16;
    // 16 * threadIdx.x nucleotides further on lies at most that many fragments further on
    u64 j = j0, hi = ext_min(j0 + 16 * (u64)threadIdx.x, j1);
    while (j < hi) {
        const u64 mid = j + (hi - j + 1) / 2;
        if (start_of(mid) <= p) j = mid;
        else hi = mid - 1;
    }
    u32 v = 0, filled = 0;
    u64 begin = start_of(j);
    while (filled < 16 && j <= j1) {
        const u64 stop = start_of(j + 1), q = p + filled;
        const u32 take = (u32)ext_min(16 - filled, stop - q);
        v |= intake_window(bases, src_pos[j] + (q - begin), take, end) >> (2 * filled);
        filled += take;
        if (q + take == stop) {
            j++;
            begin = stop;
        }
    }
    out[w] = v;
}
