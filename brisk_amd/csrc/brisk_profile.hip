// brisk_profile.hip -- per-read abundance profiles (brisk_hip_read_profile_reads / _packed): the per-position answers of one batch
// (brisk_hip_get_kmers' uint16 slots: 0 absent, 0x100 | count present) reduced to one 32-byte record per read while they are
// still on the device.  No reference counterpart (khmer's normalize-by-median and trim-low-abund are the usual tools).
//
// A read of at most `seg` slots is one wave's work (k_profile_reads): lanes stride the slots 64 at a time (coalesced uint16
// loads), the stored counts of present slots go into the wave's own 256-bin histogram in LDS, and everything the record holds
// but the run comes out of that histogram at the end -- one wave prefix scan gives both medians (the all-slots median sees the
// absent slots as that many more zeros in bin 0), the first and the last non-empty bin are min and max, sum is sum(bin * count).
// The longest run of solid slots is followed on the wave-uniform 64-bit ballot of every stride, with the open run and the best
// run in scalar registers: no per-lane scan.  A real read has one or two distinct counts: when the present lanes of a stride
// all hold one value, one lane adds the popcount (as k_spectrum does), instead of 64 LDS atomics on one address.
//
// A longer read (a chromosome is one "read" of get_kmers) is cut into segments of `seg` slots (k_profile_plan lists them); a wave
// per segment writes a partial (k_profile_segments: the segment's histogram, its solid slots, the solid run at its
// start, the one at its end and its best run), and one wave per long read folds its partials in order (k_profile_fold).
// Every store is a plain vector store; the only atomics are the LDS histogram's and k_profile_plan's two list cursors.

struct ReadProfile {  // brisk_hip_read_profile of include/brisk_hip.h (brisk_capi.hip asserts that the two agree)
    u32 n_kmers, n_present, n_solid, run_start, run_len;
    uint8_t min_present, max_present, median, median_present;
    u64 sum;
};
static_assert(sizeof(ReadProfile) == 32, "the record is four 8-byte stores");

#define PROFILE_SEG_MAX (1u << 20)  // slots of one wave's read or segment at most: 2^20 * 255 fits 32 bits, as the lanes' sums assume
#define PROFILE_MAX_SLOTS 0xffffffffull

struct ProfilePartial {  // one segment of a long read
    u32 hist[256];
    u32 n_solid;
    u32 prefix, suffix;          // solid slots at the segment's start and at its end (both the segment's length when all are solid)
    u32 best_len, best_start;    // its longest run (the first on ties), prefix and suffix included; start counted from the read's first slot
    u32 pad[3];
};
struct ProfileLong {  // a read of more than `seg` slots
    u64 read, seg0;
    u32 n_seg, pad;
};
struct ProfileSeg {
    u64 read;
    u32 j, pad;
};

struct RunState {  // wave-uniform: the compiler keeps it in scalar registers
    u32 cur_start, cur_len, best_start, best_len;
    u32 prefix;      // the run that starts at slot 0 of the range, once it has ended (segments only)
    bool at_start;   // no non-solid slot seen yet
};
__device__ __forceinline__ void run_close(RunState& s) {
    if (s.at_start) {
        s.prefix = s.cur_len;
        s.at_start = false;
    }
    if (s.cur_len > s.best_len) {  // strictly longer: the first run wins ties
        s.best_len = s.cur_len;
        s.best_start = s.cur_start;
    }
    s.cur_len = 0;
}
// one stride: bit l of `solid` is slot i0 + l, for the `width` slots of the range that the stride holds (the bits above them are 0, and
// say nothing: a run that reaches the range's last slot stays open)
__device__ __forceinline__ void run_stride(RunState& s, unsigned long long solid, u32 i0, u32 width) {
    if (solid == ~0ull) {
        if (s.cur_len == 0) s.cur_start = i0;
        s.cur_len += 64;
        return;
    }
    u32 off = 0;
    while (off < width) {
        const unsigned long long rest = solid >> off;
        if (rest & 1) {  // ones from off on (the shift filled the top with zeros, so the run ends inside the word)
            const u32 ones = (u32)__builtin_ctzll(~rest);
            if (s.cur_len == 0) s.cur_start = i0 + off;
            s.cur_len += ones;
            off += ones;
        } else {
            run_close(s);
            if (rest == 0) break;
            off += (u32)__builtin_ctzll(rest);
        }
    }
}

// The wave's histogram (lane l holds bins 4l .. 4l + 3 in h0..h3) to the record's order-free fields.  n: the read's slots; those that are not in the
// histogram (the absent ones) count as zeros for `median`.  T: u32 for one wave's slots, u64 for a folded read.
template <typename T>
__device__ __forceinline__ void profile_from_hist(T h0, T h1, T h2, T h3, u64 n, u32 lane, ReadProfile& rec) {
    const T mine = h0 + h1 + h2 + h3;
    T incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(incl, o, 64);
        if ((int)lane >= o) incl += y;
    }
    const u64 n_present = (u64)__shfl(incl, 63, 64);
    const u64 n_absent = n - n_present;
    u64 sum = (u64)h1 * (4 * lane + 1) + (u64)h2 * (4 * lane + 2) + (u64)h3 * (4 * lane + 3) + (u64)h0 * (4 * lane);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
    rec.sum = __shfl(sum, 0, 64);
    rec.n_present = (u32)n_present;
    rec.min_present = rec.max_present = rec.median = rec.median_present = 0;
    if (n == 0) return;
    // lower medians: the bin whose cumulative count is the first above the rank
    const u64 t_all = (n - 1) >> 1, t_pres = n_present ? (n_present - 1) >> 1 : 0;
    const u64 before = (u64)(incl - mine);  // present slots in the bins below this lane's
    u64 c[5] = {before, before + h0, before + h0 + h1, before + h0 + h1 + h2, before + mine};
    u32 hit_all = 0xffffffffu, hit_pres = 0xffffffffu;
#pragma unroll
    for (u32 j = 0; j < 4; j++) {
        const u32 bin = 4 * lane + j;
        const u64 lo_all = bin ? c[j] + n_absent : 0, hi_all = c[j + 1] + n_absent;
        if (lo_all <= t_all && t_all < hi_all) hit_all = bin;
        if (c[j] <= t_pres && t_pres < c[j + 1]) hit_pres = bin;
    }
    const unsigned long long b_all = __ballot(hit_all != 0xffffffffu), b_pres = __ballot(hit_pres != 0xffffffffu);
    rec.median = (uint8_t)__shfl(hit_all, __ffsll((long long)b_all) - 1, 64);  // exactly one lane holds it
    if (n_present) {
        rec.median_present = (uint8_t)__shfl(hit_pres, __ffsll((long long)b_pres) - 1, 64);
        const unsigned long long busy = __ballot(mine != 0);
        const u32 lo_bin = 4 * lane + (h0 ? 0u : h1 ? 1u : h2 ? 2u : 3u), hi_bin = 4 * lane + (h3 ? 3u : h2 ? 2u : h1 ? 1u : 0u);
        rec.min_present = (uint8_t)__shfl(lo_bin, __ffsll((long long)busy) - 1, 64);
        rec.max_present = (uint8_t)__shfl(hi_bin, 63 - __clzll((long long)busy), 64);
    }
}

__device__ __forceinline__ void profile_store(ReadProfile* __restrict__ out, const ReadProfile& rec) {
    uint2* o = reinterpret_cast<uint2*>(out);  // (a caller's array is aligned as its u64 member asks: 8 bytes)
    o[0] = uint2{rec.n_kmers, rec.n_present};
    o[1] = uint2{rec.n_solid, rec.run_start};
    o[2] = uint2{rec.run_len, (u32)rec.min_present | ((u32)rec.max_present << 8) | ((u32)rec.median << 16) | ((u32)rec.median_present << 24)};
    o[3] = uint2{(u32)rec.sum, (u32)(rec.sum >> 32)};
}

// Slots [begin, begin + n) of `slots` into the wave's histogram (zeroed here) and the run state; returns the solid slots.
// n <= PROFILE_SEG_MAX.  first_slot: what slot `begin` is called in run positions.
__device__ __forceinline__ u32 profile_pass(const uint16_t* __restrict__ slots, u64 begin, u32 n, u32 first_slot, u32 solid_min, u32* hist, u32 lane,
                                            RunState& rs) {
    reinterpret_cast<uint4*>(hist)[lane] = uint4{0, 0, 0, 0};
    wave_sync();
    u32 n_solid = 0;
    for (u32 i0 = 0; i0 < n; i0 += 64) {
        const bool valid = n - i0 > lane;
        const u32 v = valid ? (u32)slots[begin + i0 + lane] : 0u;
        const bool present = (v & 0x100u) != 0;
        const u32 c = v & 0xffu;
        const unsigned long long pres = __ballot(present);
        const unsigned long long solid = __ballot(present && c >= solid_min);
        n_solid += (u32)__popcll(solid);
        if (pres) {
            const u32 first = (u32)__ffsll((long long)pres) - 1;
            const u32 lead = (u32)__builtin_amdgcn_readlane((int)c, (int)first);
            if (__ballot(present && c != lead) == 0) {  // one value in the whole stride: one add
                if (lane == first) atomicAdd(&hist[lead], (u32)__popcll(pres));
            } else if (present) {
                atomicAdd(&hist[c], 1u);
            }
        }
        run_stride(rs, solid, first_slot + i0, min(n - i0, 64u));
    }
    wave_sync();
    return n_solid;
}

// One wave per read of at most `seg` slots; longer reads are left to the segment kernels (k_profile_plan lists them).  slot_base is
// kmers_packed_impl's (k_slot_apply): the first slot of read r is slot_base[r] + starts[r].
__global__ void __launch_bounds__(256) k_profile_reads(const uint16_t* __restrict__ slots, const u64* __restrict__ starts, const u64* __restrict__ slot_base,
                                                       u64 n_reads, u32 k, u32 solid_min, u32 seg, ReadProfile* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) u32 s_hist[4][256];
    const u32 lane = threadIdx.x & 63, wib = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform, and the compiler knows
    u32* hist = s_hist[wib];
    const u64 n_waves = (u64)gridDim.x * 4;
    for (u64 r = (u64)blockIdx.x * 4 + wib; r < n_reads; r += n_waves) {
        const u64 n64 = read_slots(starts, r, k);
        if (n64 > seg) continue;  // (wave-uniform)
        const u32 n = (u32)n64;
        ReadProfile rec{};
        rec.n_kmers = n;
        if (n) {
            RunState rs{0, 0, 0, 0, 0, false};
            rec.n_solid = profile_pass(slots, slot_base[r] + starts[r], n, 0, solid_min, hist, lane, rs);
            run_close(rs);
            rec.run_start = rs.best_len ? rs.best_start : 0;
            rec.run_len = rs.best_len;
            const uint4 h = reinterpret_cast<const uint4*>(hist)[lane];
            profile_from_hist<u32>(h.x, h.y, h.z, h.w, n, lane, rec);
            wave_sync();  // the next read zeroes the histogram
        }
        if (lane == 0) profile_store(out + r, rec);
    }
}

// ctr[0] += segments, ctr[1] += reads of more than `seg` slots, ctr[2] |= 1 when a read has more than 2^32 - 1 slots
__global__ void __launch_bounds__(256) k_profile_count_long(const u64* __restrict__ starts, u64 n_reads, u32 k, u32 seg, unsigned long long* __restrict__ ctr) {
    unsigned long long segs = 0, longs = 0;
    bool too_long = false;
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (u64)gridDim.x * blockDim.x) {
        const u64 n = read_slots(starts, r, k);
        if (n > PROFILE_MAX_SLOTS) too_long = true;
        else if (n > seg) {
            segs += (n + seg - 1) / seg;
            longs++;
        }
    }
    if (too_long) atomicOr(ctr + 2, 1ull);
    if (segs) {
        atomicAdd(ctr, segs);
        atomicAdd(ctr + 1, longs);
    }
}
// the long reads and their segments as lists (in no particular order): ctr[3] and ctr[4] are the two cursors, zero on entry
__global__ void __launch_bounds__(256) k_profile_plan(const u64* __restrict__ starts, u64 n_reads, u32 k, u32 seg, unsigned long long* __restrict__ ctr,
                                                      ProfileLong* __restrict__ longs, u64 cap_longs, ProfileSeg* __restrict__ segs, u64 cap_segs) {
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (u64)gridDim.x * blockDim.x) {
        const u64 n = read_slots(starts, r, k);
        if (n <= seg || n > PROFILE_MAX_SLOTS) continue;
        const u64 n_seg = (n + seg - 1) / seg;
        const u64 s0 = atomicAdd(ctr + 3, (unsigned long long)n_seg), li = atomicAdd(ctr + 4, 1ull);
        if (li >= cap_longs || s0 + n_seg > cap_segs) continue;  // (cannot happen: the capacities are k_profile_count_long's counts of the same table)
        longs[li] = ProfileLong{r, s0, (u32)n_seg, 0};
        for (u64 j = 0; j < n_seg; j++) segs[s0 + j] = ProfileSeg{r, (u32)j, 0};
    }
}

// one wave per segment of a long read
__global__ void __launch_bounds__(256) k_profile_segments(const uint16_t* __restrict__ slots, const u64* __restrict__ starts, const u64* __restrict__ slot_base, u32 k,
                                                          u32 solid_min, u32 seg, const ProfileSeg* __restrict__ segs, u64 n_segs, ProfilePartial* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) u32 s_hist[4][256];
    const u32 lane = threadIdx.x & 63, wib = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform, and the compiler knows
    u32* hist = s_hist[wib];
    const u64 n_waves = (u64)gridDim.x * 4;
    for (u64 s = (u64)blockIdx.x * 4 + wib; s < n_segs; s += n_waves) {
        const ProfileSeg d = segs[s];
        const u64 n_read = read_slots(starts, d.read, k);
        const u64 first = (u64)d.j * seg;
        const u32 n = (u32)min((u64)seg, n_read - first);
        RunState rs{0, 0, 0, 0, 0, true};
        const u32 n_solid = profile_pass(slots, slot_base[d.read] + starts[d.read] + first, n, (u32)first, solid_min, hist, lane, rs);
        const u32 suffix = rs.cur_len;  // the run still open at the end
        run_close(rs);                  // (a segment without a non-solid slot: prefix = suffix = n)
        const uint4 h = reinterpret_cast<const uint4*>(hist)[lane];
        ProfilePartial* p = part + s;
        reinterpret_cast<uint4*>(p->hist)[lane] = h;
        if (lane == 0) {
            uint4* tail = reinterpret_cast<uint4*>(&p->n_solid);
            tail[0] = uint4{n_solid, rs.prefix, suffix, rs.best_len};
            tail[1] = uint4{rs.best_start, 0, 0, 0};
        }
        wave_sync();
    }
}

// one wave per long read: its partials folded in segment order
__global__ void __launch_bounds__(256) k_profile_fold(const u64* __restrict__ starts, u32 k, u32 seg, const ProfileLong* __restrict__ longs, u64 n_longs,
                                                      const ProfilePartial* __restrict__ part, ReadProfile* __restrict__ out) {
    const u32 lane = threadIdx.x & 63, wib = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform, and the compiler knows
    const u64 n_waves = (u64)gridDim.x * 4;
    for (u64 li = (u64)blockIdx.x * 4 + wib; li < n_longs; li += n_waves) {
        const ProfileLong d = longs[li];
        const u64 n = read_slots(starts, d.read, k);
        u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0, n_solid = 0;
        u32 carry_len = 0, carry_start = 0, best_len = 0, best_start = 0;  // carry: the run open at the end of the segments so far
        for (u32 j = 0; j < d.n_seg; j++) {
            const ProfilePartial* p = part + d.seg0 + j;
            const uint4 h = reinterpret_cast<const uint4*>(p->hist)[lane];
            h0 += h.x; h1 += h.y; h2 += h.z; h3 += h.w;
            const uint4 t0 = *reinterpret_cast<const uint4*>(&p->n_solid);  // n_solid, prefix, suffix, best_len (the same in every lane)
            const u32 seg_best_start = p->best_start;
            const u64 seg_begin = (u64)j * seg;
            const u32 len = (u32)min((u64)seg, n - seg_begin);
            n_solid += t0.x;
            if (t0.y) {
                if (carry_len == 0) carry_start = (u32)seg_begin;
                carry_len += t0.y;
            }
            if (t0.y == len) continue;  // solid from end to end: the run stays open
            if (carry_len > best_len) { best_len = carry_len; best_start = carry_start; }
            if (t0.w > best_len) { best_len = t0.w; best_start = seg_best_start; }  // (its prefix run is no longer than the carry just seen; its suffix run keeps its start)
            carry_len = t0.z;
            carry_start = (u32)(seg_begin + len - t0.z);
        }
        if (carry_len > best_len) { best_len = carry_len; best_start = carry_start; }
        ReadProfile rec{};
        rec.n_kmers = (u32)n;
        rec.n_solid = (u32)n_solid;
        rec.run_len = best_len;
        rec.run_start = best_len ? best_start : 0;
        profile_from_hist<u64>(h0, h1, h2, h3, n, lane, rec);
        if (lane == 0) profile_store(out + d.read, rec);
    }
}
