// brisk_pairs.hip -- paired-end bookkeeping in the interval domain (brisk_hip_fragment_intervals / brisk_hip_pair_intervals /
// brisk_hip_compose_intervals / brisk_hip_extract_pairs_packed and the composed brisk_hip_trim_pairs_* / brisk_hip_clean_pairs_*).
// No reference counterpart (khmer's extract-paired-reads and Trimmomatic's paired mode are the usual tools).  A paired stream is
// interleaved: reads 2p and 2p + 1 are the mates of pair p; a read is kept when its interval has len > 0, and nothing else encodes
// the state of a pair.  Included by brisk_kernels.hip, after brisk_extract.hip (ReadInterval) and brisk_intake.hip (IntakeFragment).
//
// k_fragment_check      one lane per row of an intake fragment table: the first row with read >= n_reads, or that stands before its
//                       predecessor (by read, then by position), by one atomicMin per wave that found one
// k_fragment_intervals  one lane per read: its rows are found by a search over the (checked) table, the first longest one is its interval
// k_pair_intervals      one lane per pair: the pair decision (each / all / any) over the mates' intervals
// k_compose_check       one lane per kept read of the inner cut: inner leaves outer, or the index leaves the table or does not ascend
// k_compose_intervals   one lane per input read: found in the index, its inner interval moves into the outer one's frame; else {0,0}
// k_pair_split          eight pairs per lane: the intervals of intact pairs to one table, those of singles to another, six counters
//                       (reduced in the wave, one atomic add per wave and counter, into one of 64 rows that the host sums); with a
//                       read table, k_extract_block's two flags
// k_rebase_starts       one lane per row: a read table made to begin at 0
//
// Every output row is stored once, by a plain store.

#define PAIR_EACH 0u
#define PAIR_ALL 1u
#define PAIR_ANY 2u

// the smallest value of the wave's lanes (all 64 lanes of the wave run this), in every lane that reads lane 0's
__device__ __forceinline__ u64 pair_wave_min(u64 v) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 y = __shfl_down(v, o, 64);
        v = y < v ? y : v;
    }
    return v;
}
__device__ __forceinline__ u64 pair_wave_sum(u64 v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// flags[0]: the first bad row (~0: none)
__global__ void __launch_bounds__(256) k_fragment_check(const IntakeFragment* __restrict__ frags, u64 n_frags, u64 n_reads, unsigned long long* __restrict__ flags) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 bad = ~0ull;
    if (j < n_frags) {
        const IntakeFragment f = frags[j];
        bool wrong = f.read >= n_reads;
        if (!wrong && j) {
            const IntakeFragment g = frags[j - 1];
            wrong = g.read > f.read || (g.read == f.read && g.start >= f.start);
        }
        if (wrong) bad = j;
    }
    bad = pair_wave_min(bad);
    if ((threadIdx.x & 63) == 0 && bad != ~0ull) atomicMin(flags, (unsigned long long)bad);
}

// the table is checked: ascending by read, then by position, every read < n_reads
__global__ void __launch_bounds__(256) k_fragment_intervals(const IntakeFragment* __restrict__ frags, u64 n_frags, u64 n_reads, ReadInterval* __restrict__ out) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    u64 lo = 0, hi = n_frags;  // the first row with read >= r
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (frags[mid].read < r) lo = mid + 1;
        else hi = mid;
    }
    ReadInterval best;
    best.start = best.len = 0;
    for (u64 j = lo; j < n_frags; j++) {
        const IntakeFragment f = frags[j];
        if (f.read != r) break;
        if (f.len > best.len) {  // (strictly: of equal lengths the first one stays)
            best.start = f.start;
            best.len = f.len;
        }
    }
    out[r] = best;
}

// out may be each: a lane reads its pair before it writes it, and no other lane touches it
__global__ void __launch_bounds__(256) k_pair_intervals(const ReadInterval* each, const ReadInterval* __restrict__ whole, u64 n_pairs, u32 mode, ReadInterval* out) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    ReadInterval a = each[2 * p], b = each[2 * p + 1];
    const ReadInterval none = {0, 0};
    if (mode == PAIR_ALL) {
        if (!a.len || !b.len) a = b = none;
    } else if (mode == PAIR_ANY) {
        if (a.len || b.len) {
            a = whole[2 * p];
            b = whole[2 * p + 1];
            if (!a.len) a = none;
            if (!b.len) b = none;
        } else {
            a = b = none;
        }
    }  // (PAIR_EACH: the rows as they are)
    out[2 * p] = a;
    out[2 * p + 1] = b;
}

// flags[0]: the first kept read j whose inner interval leaves the outer one, or whose index[j] >= n_reads (~0: none);
// flags[1]: the first j with index[j] <= index[j - 1] (~0: none)
__global__ void __launch_bounds__(256) k_compose_check(const ReadInterval* __restrict__ outer, u64 n_reads, const ReadInterval* __restrict__ inner, const u64* __restrict__ index,
                                                       u64 n_kept, unsigned long long* __restrict__ flags) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 bad = ~0ull, unordered = ~0ull;
    if (j < n_kept) {
        const u64 r = index[j];
        if (r >= n_reads) {
            bad = j;
        } else {
            const ReadInterval v = inner[j];
            if ((u64)v.start + v.len > outer[r].len) bad = j;
        }
        if (j && index[j - 1] >= r) unordered = j;
    }
    bad = pair_wave_min(bad);
    unordered = pair_wave_min(unordered);
    if ((threadIdx.x & 63) == 0) {
        if (bad != ~0ull) atomicMin(flags, (unsigned long long)bad);
        if (unordered != ~0ull) atomicMin(flags + 1, (unsigned long long)unordered);
    }
}

// the inputs are checked: index ascends strictly and stays below n_reads, inner[j] lies inside outer[index[j]]
__global__ void __launch_bounds__(256) k_compose_intervals(const ReadInterval* __restrict__ outer, u64 n_reads, const ReadInterval* __restrict__ inner, const u64* __restrict__ index,
                                                           u64 n_kept, ReadInterval* __restrict__ out) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    u64 lo = 0, hi = n_kept;  // the first j with index[j] >= r
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (index[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    ReadInterval v;
    v.start = v.len = 0;
    if (lo < n_kept && index[lo] == r) {
        const ReadInterval in = inner[lo];
        if (in.len) {
            v.start = outer[r].start + in.start;
            v.len = in.len;
        }
    }
    out[r] = v;
}

// PAIR_ITEMS pairs a lane, a block's lanes side by side in each round (k_extract_block's shape), so that a wave has eight times the
// pairs to put behind one atomic; and the adds of different blocks go to PAIR_CTR_ROWS rows of counters, a cache line each, which
// the host sums.  (One pair a lane and one row: 2.3 M adds to six addresses, 23 ms for 25 M pairs where the bytes take under one.)
#define PAIR_ITEMS 8
#define PAIR_CTR_ROWS 64
// ctr[row][0..5]: pairs kept, singles that are mate 1, singles that are mate 2, pairs dropped, nucleotides of pairs, nucleotides of
// singles; starts (may be NULL: nothing is checked): flags[0] the first read whose interval leaves it (~0 none), flags[1] starts[]
// does not ascend somewhere -- k_extract_block's two, so that the host can refuse before either stream is written
__global__ void __launch_bounds__(256) k_pair_split(const ReadInterval* __restrict__ iv, u64 n_pairs, const u64* __restrict__ starts, ReadInterval* __restrict__ iv_pairs,
                                                    ReadInterval* __restrict__ iv_singles, unsigned long long* __restrict__ ctr, unsigned long long* __restrict__ flags) {
    const u64 base = (u64)blockIdx.x * 256 * PAIR_ITEMS;
    u64 c[6] = {0, 0, 0, 0, 0, 0};
    u64 bad = ~0ull, descends = 0;
    for (int i = 0; i < PAIR_ITEMS; i++) {
        const u64 p = base + (u64)i * 256 + threadIdx.x;
        if (p >= n_pairs) continue;
        const ReadInterval a = iv[2 * p], b = iv[2 * p + 1];
        if (starts) {
            const u64 s0 = starts[2 * p], s1 = starts[2 * p + 1], s2 = starts[2 * p + 2];
            if (s1 < s0 || s2 < s1) descends = 1;
            u64 mine = ~0ull;
            if (s1 >= s0 && (u64)a.start + a.len > s1 - s0) mine = 2 * p;
            else if (s2 >= s1 && (u64)b.start + b.len > s2 - s1) mine = 2 * p + 1;
            bad = mine < bad ? mine : bad;
        }
        const ReadInterval none = {0, 0};
        const bool ka = a.len != 0, kb = b.len != 0, both = ka && kb;
        iv_pairs[2 * p] = both ? a : none;
        iv_pairs[2 * p + 1] = both ? b : none;
        iv_singles[2 * p] = ka && !kb ? a : none;
        iv_singles[2 * p + 1] = kb && !ka ? b : none;
        c[0] += both;
        c[1] += ka && !kb;
        c[2] += kb && !ka;
        c[3] += !ka && !kb;
        c[4] += both ? (u64)a.len + b.len : 0;
        c[5] += both ? 0 : (u64)a.len + b.len;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) c[i] = pair_wave_sum(c[i]);
    bad = pair_wave_min(bad);
    descends = pair_wave_sum(descends);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* row = ctr + (size_t)(blockIdx.x % PAIR_CTR_ROWS) * 8;
#pragma unroll
        for (int i = 0; i < 6; i++)
            if (c[i]) atomicAdd(row + i, (unsigned long long)c[i]);
        if (bad != ~0ull) atomicMin(flags, (unsigned long long)bad);
        if (descends) atomicOr(flags + 1, 1ull);
    }
}

// out[i] = in[i] - in[0]'s value `lo`, i in [0, n_rows)
__global__ void __launch_bounds__(256) k_rebase_starts(const u64* __restrict__ in, u64 n_rows, u64 lo, u64* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rows) out[i] = in[i] - lo;
}
