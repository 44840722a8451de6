// brisk_insert.hip -- the index: partition directory, arena, k_insert (one wave per partition), bucket bits, stats.
// Included by brisk_kernels.hip (one translation unit).
// ===========================================================================
// k_insert: persistent workgroups, each walking a strided share of the touched
// partitions.  Per partition (per chunk of at most WI_MAX_INST k-mer instances):
//   0. every k-mer instance of the chunk's records is expanded to its 128-bit
//      entry key in LDS (one wave per record, one lane per k-mer);
//   1. the instances are de-duplicated in an LDS table whose slots hold the index
//      of the first instance and a multiplicity;
//   2. the partition's existing entries stream through the table: a hit adds the
//      multiplicity to the entry's count (uint8_t, wraps; counter.cpp:264-268 -- or, in a saturating index, stops at 255);
//   3. unmatched table entries are appended as new entries (count = multiplicity).
// Storage per partition: keys[] (u128) and counts[] (u8) in a bump-allocated arena.
// A partition that outgrows its slice moves to a fresh one taken from the
// workgroup's private arena chunk, so the global cursor sees one atomic per
// ARENA_CHUNK entries.  nb_kmers / nb_buckets are reductions done at stats() time:
// the kernel has no same-address global atomics on its data path.
#ifndef ARENA_CHUNK
#define ARENA_CHUNK 16384u   // entries a persistent wave takes from the global cursor at a time
#endif
// k_insert is bound by each wave's own serial instruction stream (LDS round trips, short dependent
// chains), so throughput follows the number of resident waves: chunks of 256 instances keep LDS at
// 10 KB and registers at 128 per wave => 4 waves per SIMD (512-instance chunks: 16 KB, 201 registers,
// 2 waves per SIMD, 61 ms instead of 50 ms on the 50M-read job; 128-instance chunks spill and split
// too many partitions: 84 ms).
#ifndef INSERT_SLOTS
#define INSERT_SLOTS 8192u   // private allocator slots: an upper bound of the persistent waves (256 CUs x 4 SIMDs x 8 waves)
#endif
#ifndef WI_WAVES_PER_EU
#define WI_WAVES_PER_EU 4
#endif
// Phase timers of k_insert (debug builds only: -DBRISK_PHASE_PROF): s_memtime at phase boundaries, scalar arithmetic,
// one atomic per phase and wave at the end.  Wall cycles of a wave, so they include what it waits for.
#ifdef BRISK_PHASE_PROF
__device__ unsigned long long g_phase[16];
#define PHASE_DECL unsigned long long ph_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long ph_last = __builtin_amdgcn_s_memtime(); u32 dbg_cnt[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define PHASE(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); ph_acc[i] += t_ - ph_last; ph_last = t_; }  /* phase i ends here */
__device__ unsigned long long g_cnt[16];
#define PHASE_FLUSH { PHASE(10) if (threadIdx.x == 0) { _Pragma("unroll") for (int q_ = 0; q_ < 12; q_++) atomicAdd(&g_phase[q_], ph_acc[q_]); \
                                                         _Pragma("unroll") for (int q_ = 0; q_ < 16; q_++) atomicAdd(&g_cnt[q_], (unsigned long long)dbg_cnt[q_]); } }
#define CNT(i, v) dbg_cnt[i] += (v);
#else
#define PHASE_DECL
#define PHASE(i)
#define PHASE_FLUSH
#define CNT(i, v)
#endif
struct IndexDev {
    u64* keys;                   // 2 u64 per entry
    uint8_t* counts;
    DirEnt* dir;
    unsigned long long* cursor;  // arena entries handed out
    u32* bucket_bits;            // one bit per bucket id
    unsigned long long* stats;   // [3] garbage entries (abandoned slices)
    unsigned long long* slot_cur;  // per persistent workgroup: private chunk [cur, end)
    unsigned long long* slot_end;
    u32* ids;                    // entry-id mode only: stable dense id of every entry (insertion order)
    unsigned long long arena_cap;  // entries the arena can hold
    u32* err;                    // sticky violation bits: 1 scatter slot out of range, 2 arena exhausted, 4 chunk overflow
    u32 bits_check;              // few buckets (2b < 20): read a bucket-bitmap word before or-ing into it
    u32 huge_at;                 // partitions of more k-mer instances than this are left to k_insert_huge (0: none are)
    u32 key_words;               // u64 words per stored key: 1 where [routing id low bits | compacted k-mer | idx'] fits 64 bits
                                 // (shift + 2(k-b) + 6 <= 64: k31 b14, k31 b11, ...: 9 bytes per entry instead of 17), else 2
};
// An entry's count byte from an exact sum or multiplicity.  SAT false (the default, as the reference's uint8_t counter): its low 8
// bits.  SAT true (brisk_hip_options.count_mode == BRISK_HIP_COUNTS_SATURATE): clamped to 255.  Saturating addition of
// non-negative numbers is associative, so every stage may clamp what it hands on; the wider sums in between are exact.
// A compile-time parameter of the bodies: the default instantiations are instruction for instruction what they were.
template <bool SAT>
__device__ __forceinline__ u32 count8(u32 x) {
    return SAT ? (x < 255u ? x : 255u) : (x & 0xffu);
}
// an entry's key in the arena (KW: the word count where the caller knows it at compile time, 0: from ix)
template <u32 KW = 0>
__device__ __forceinline__ u128x load_key(const IndexDev& ix, unsigned long long at) {
    if ((KW ? KW : ix.key_words) == 1) return u128x{ix.keys[at], 0};
    return u128x{ix.keys[2 * at], ix.keys[2 * at + 1]};
}
template <u32 KW = 0>
__device__ __forceinline__ void store_key(const IndexDev& ix, unsigned long long at, u64 lo, u64 hi) {
    if ((KW ? KW : ix.key_words) == 1) {
        ix.keys[at] = lo;
    } else {
        ix.keys[2 * at] = lo;
        ix.keys[2 * at + 1] = hi;
    }
}
template <u32 KW = 0>
__device__ __forceinline__ void move_key(const IndexDev& ix, unsigned long long dst, unsigned long long src) {
    if ((KW ? KW : ix.key_words) == 1) {
        ix.keys[dst] = ix.keys[src];
    } else {
        ix.keys[2 * dst] = ix.keys[2 * src];
        ix.keys[2 * dst + 1] = ix.keys[2 * src + 1];
    }
}

// k_insert: ONE WAVE per partition, no workgroup barriers: every wave is an
// independent stream of partitions, so a CU keeps ~10 of them in flight and their
// LDS / HBM latencies overlap.  Sized for partitions of a few hundred k-mer
// instances (part_bits = 24 at b = 14: 16 buckets per partition).
#ifndef WI_MAX_INST
#define WI_MAX_INST 256     // k-mer instances per chunk
#endif
#define WI_TABLE (2 * WI_MAX_INST)   // LDS table slots (load <= 0.5)
static_assert(WI_MAX_INST % 256 == 0 && WI_MAX_INST <= 1024, "chunk size: whole 32-bit words of record marks per lane, 10-bit instance index");
#define WI_MAX_REC 64       // records per chunk: one per lane
#define WI_CNT_SHIFT 10     // table word = [MATCHED | multiplicity (21 b) | instance (10 b)]
#define WI_IDX_MASK 0x3ffu
#define wave_sync() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")

// record words of the calling lane's record (lane r < n loads record first+r), 5 words at most
struct RecRegs {
    u64 w0, w1, w2, w3, w4;
};
__device__ __forceinline__ RecRegs load_rec_regs(const BriskParams& P, const u64* __restrict__ rec, u32 first, u32 n, u32 lane) {
    RecRegs r{0, 0, 0, 0, 0};
    if (lane < n) {
        const u64* c = rec + (u64)(first + lane) * P.stride;
        r.w0 = c[0];
        r.w1 = c[1];
        if (P.stride > 2) r.w2 = c[2];
        if (P.stride > 3) r.w3 = c[3];
        if (P.stride > 4) r.w4 = c[4];
    }
    return r;
}
// Where a partition's records are.  Classic (bin_cap == 0): `rec` holds all records in partition order, a partition's at
// [r_begin, r_begin + n_rec).  Binned (the scan wrote every record straight into its partition's bin):
// record i of partition `part` is rec[part * bin_cap + i] for i < bin_cap, and ovf[r_begin + i - bin_cap] beyond (the few
// partitions that overflow their bin; r_begin is then the partition's offset among the overflow records).
struct RecSrc {
    u64* rec;
    const u64* ovf;
    u32 bin_cap;
};
__device__ __forceinline__ RecRegs load_part_recs(const BriskParams& P, const RecSrc& src, u32 part, u32 r_begin, u32 first, u32 n, u32 lane) {
    if (!src.bin_cap) return load_rec_regs(P, src.rec, first, n, lane);
    RecRegs r{0, 0, 0, 0, 0};
    if (lane < n) {
        const u32 i = first - r_begin + lane;
        const u64* c = i < src.bin_cap ? src.rec + ((u64)part * src.bin_cap + i) * P.stride : src.ovf + ((u64)r_begin + i - src.bin_cap) * P.stride;
        r.w0 = c[0];
        r.w1 = c[1];
        if (P.stride > 2) r.w2 = c[2];
        if (P.stride > 3) r.w3 = c[3];
        if (P.stride > 4) r.w4 = c[4];
    }
    return r;
}
// Inclusive scans over the 64 lanes on the DPP network: row_shr 1,2,4,8 inside each row of 16, then row_bcast15
// and row_bcast31 carry the row totals over.  Lanes without a source keep the identity 0.  Full EXEC mask only.
#define WAVE_SCAN_STEP(x, OP, CTRL, ROW_MASK)                                                         \
    {                                                                                                 \
        const u32 y_ = (u32)__builtin_amdgcn_update_dpp(0, (int)(x), CTRL, ROW_MASK, 0xf, false); \
        x = OP(x, y_);                                                                                \
    }
__device__ __forceinline__ u32 op_add_u32(u32 a, u32 b) { return a + b; }
__device__ __forceinline__ u32 op_max_u32(u32 a, u32 b) { return a > b ? a : b; }
__device__ __forceinline__ u32 wave_incl_scan(u32 x, u32 /*lane*/) {
    WAVE_SCAN_STEP(x, op_add_u32, 0x111, 0xf)  // row_shr:1
    WAVE_SCAN_STEP(x, op_add_u32, 0x112, 0xf)  // row_shr:2
    WAVE_SCAN_STEP(x, op_add_u32, 0x114, 0xf)  // row_shr:4
    WAVE_SCAN_STEP(x, op_add_u32, 0x118, 0xf)  // row_shr:8
    WAVE_SCAN_STEP(x, op_add_u32, 0x142, 0xa)  // row_bcast:15 -> rows 1, 3
    WAVE_SCAN_STEP(x, op_add_u32, 0x143, 0xc)  // row_bcast:31 -> rows 2, 3
    return x;
}
__device__ __forceinline__ u32 wave_incl_max_scan(u32 x) {
    WAVE_SCAN_STEP(x, op_max_u32, 0x111, 0xf)
    WAVE_SCAN_STEP(x, op_max_u32, 0x112, 0xf)
    WAVE_SCAN_STEP(x, op_max_u32, 0x114, 0xf)
    WAVE_SCAN_STEP(x, op_max_u32, 0x118, 0xf)
    WAVE_SCAN_STEP(x, op_max_u32, 0x142, 0xa)
    WAVE_SCAN_STEP(x, op_max_u32, 0x143, 0xc)
    return x;
}
// OR over all 64 lanes, the same value in every lane (through lane 63 and a scalar register).  Full EXEC mask only.
__device__ __forceinline__ u32 op_or_u32(u32 a, u32 b) { return a | b; }
__device__ __forceinline__ u32 wave_or_all(u32 x) {
    WAVE_SCAN_STEP(x, op_or_u32, 0x111, 0xf)
    WAVE_SCAN_STEP(x, op_or_u32, 0x112, 0xf)
    WAVE_SCAN_STEP(x, op_or_u32, 0x114, 0xf)
    WAVE_SCAN_STEP(x, op_or_u32, 0x118, 0xf)
    WAVE_SCAN_STEP(x, op_or_u32, 0x142, 0xa)
    WAVE_SCAN_STEP(x, op_or_u32, 0x143, 0xc)
    return (u32)__builtin_amdgcn_readlane((int)x, 63);
}
// value of the previous lane (0 for lane 0)
__device__ __forceinline__ u32 wave_prev_lane(u32 x) { return (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x138, 0xf, 0xf, false); }  // wave_shr:1

#define WI_TS (WI_TABLE / 64)      // table words per lane

// k-mer j of record words in LDS, branch-free (every load is unconditional so that the
// unrolled instances of a lane keep their LDS reads in flight together)
template <u32 NW>  // NW > 0: compile-time record width; 0: P.nw
__device__ __forceinline__ u128x record_kmer_lds(const BriskParams& P, const u64* c, u32 n, u32 j) {
    const u32 s = 2 * (n - 1 - j);
    const u32 ws = s >> 6, bs = s & 63;
    const u32 last = (NW ? NW : P.nw) - 1;
    const u64 t0 = c[ws < last ? ws : last], t1 = c[ws + 1 < last ? ws + 1 : last], t2 = c[ws + 2 < last ? ws + 2 : last];
    const u64 a0 = ws <= last ? t0 : 0, a1 = ws + 1 <= last ? t1 : 0, a2 = ws + 2 <= last ? t2 : 0;
    u128x r;
    r.lo = bs ? ((a0 >> bs) | (a1 << (64 - bs))) : a0;
    r.hi = bs ? ((a1 >> bs) | (a2 << (64 - bs))) : a1;
    return and128(r, mask128(2 * P.kb));
}

#define WI_BATCH 64u   // partitions a wave takes per work-counter atomic (same-address atomics serialise device-wide)

// NI-instances-per-lane body of the expand + de-duplicate phases (NI = 4 when the
// chunk has <= 256 instances, else 8: all NI instances of a lane are in flight together)
template <u32 NI, u32 NW, bool SAT>
__device__ __forceinline__ void expand_and_dedupe(const BriskParams& P, u32 lane, u32 ninst, u32 tsize, const u64* s_rec, const u32* s_pref,
                                                  const uint8_t* s_irec, const u32* s_rmult, u64* s_key, u32* s_tab) {
    u64 klo[NI], khi[NI];
    u32 hh[NI], mult[NI];
    u32 rix[NI];
#pragma unroll
    for (u32 it = 0; it < NI; it++) {
        const u32 i = it * 64 + lane;
        rix[it] = s_irec[i < ninst ? i : 0];
    }
#pragma unroll
    for (u32 it = 0; it < NI; it++) {
        const u32 i = it * 64 + lane;
        const u32 r = rix[it];
        const u64* c = s_rec + r * (NW ? NW + 1 : P.stride);
        const u64 hdr = c[NW ? NW : P.nw];
        const u32 j = i < ninst ? i - s_pref[r] : 0;
        const u128x key = make_key(P, hdr_bucket(hdr), record_kmer_lds<NW>(P, c, hdr_n(hdr), j), hdr_idx0(hdr) + j);
        klo[it] = key.lo;
        khi[it] = key.hi;
        hh[it] = hash_key32(key) & (tsize - 1);
        mult[it] = count8<SAT>(s_rmult[r]) << WI_CNT_SHIFT;  // counts wrap at 256 (SAT: stop at 255): so may the multiplicities
        if (i < ninst) {
            s_key[2 * i] = key.lo;
            s_key[2 * i + 1] = key.hi;
        }
    }
    wave_sync();
    // de-duplicate: all of a lane's instances probe in lockstep rounds
    u32 pending = 0;
#pragma unroll
    for (u32 it = 0; it < NI; it++)
        if (it * 64 + lane < ninst) pending |= 1u << it;
    while (__any(pending != 0)) {
        u32 old[NI];
#pragma unroll
        for (u32 it = 0; it < NI; it++) {
            old[it] = EMPTY_SLOT;
            if (pending >> it & 1) old[it] = atomicCAS(&s_tab[hh[it]], EMPTY_SLOT, (it * 64 + lane) | mult[it]);
        }
        u64 olo[NI], ohi[NI];
#pragma unroll
        for (u32 it = 0; it < NI; it++) {
            const u32 oi = old[it] == EMPTY_SLOT ? 0 : (old[it] & WI_IDX_MASK);
            olo[it] = s_key[2 * oi];
            ohi[it] = s_key[2 * oi + 1];
        }
#pragma unroll
        for (u32 it = 0; it < NI; it++) {
            if (pending >> it & 1) {
                if (old[it] == EMPTY_SLOT) {
                    pending &= ~(1u << it);
                } else if (olo[it] == klo[it] && ohi[it] == khi[it]) {
                    atomicAdd(&s_tab[hh[it]], mult[it]);
                    pending &= ~(1u << it);
                } else {
                    hh[it] = (hh[it] + 1) & (tsize - 1);
                }
            }
        }
    }
}

// ---- compile-time record geometry (the common parameter sets): records are laid down in LDS as 32-bit words of
// (C << 6) followed by one packed info word, and k-mer j's 128-bit entry key is five adjacent words funnel-shifted
// (v_alignbit) by s = 2(n-1-j): bits [0,6) of the window then take idx', bits above 2kb+6 the routing id's low bits.
// 36 vector instructions per instance instead of 73 with the u64 shifts of record_kmer_lds + make_key + shl128.
template <u32 NW>
struct RecGeom {
    static constexpr u32 CW = 2 * NW + 1;     // words of C << 6
    static constexpr u32 RS = 2 * NW + 3;     // record stride in words (odd: lanes on different records hit different banks)
    static constexpr u32 INFO = 2 * NW + 1;   // [pref:10 | n:8 | idx0:8 | routing id low bits:6]
};
template <u32 NW>
__device__ __forceinline__ void store_rec_words(u32* dst, const RecRegs& rr, u32 info) {
    const u64 c0 = rr.w0, c1 = NW > 1 ? rr.w1 : 0, c2 = NW > 2 ? rr.w2 : 0, c3 = NW > 3 ? rr.w3 : 0;
    const u64 s0 = c0 << 6, s1 = (c1 << 6) | (c0 >> 58), s2 = (c2 << 6) | (c1 >> 58), s3 = (c3 << 6) | (c2 >> 58);
    const u32 top = (u32)((NW == 1 ? c0 : NW == 2 ? c1 : NW == 3 ? c2 : c3) >> 58);
    dst[0] = (u32)s0;
    dst[1] = (u32)(s0 >> 32);
    if (NW > 1) { dst[2] = (u32)s1; dst[3] = (u32)(s1 >> 32); }
    if (NW > 2) { dst[4] = (u32)s2; dst[5] = (u32)(s2 >> 32); }
    if (NW > 3) { dst[6] = (u32)s3; dst[7] = (u32)(s3 >> 32); }
    dst[2 * NW] = top;
    dst[RecGeom<NW>::INFO] = info;
    dst[RecGeom<NW>::INFO + 1] = 0;  // read (and shifted out) by the last k-mer's window
}
// What a lane keeps of its instances for the append (register arrays, compile-time indices only): their keys, the table
// slot each ended up in, and which of them CREATED their slot (the first copy of a key).
template <u32 NIMAX>
struct LaneInst {
    u64 klo[NIMAX], khi[NIMAX];
    u32 hh[NIMAX];
    u32 won;
};
// The entry key of instance i (i >= ninst: of the record's instance 0, never used) cut out of its record's words at `base`.
template <u32 NW, u32 KB, u32 SHIFT>
__device__ __forceinline__ void cut_key(const u32* base, u32 i, u32 ninst, u64* lo_out, u64* hi_out) {
    constexpr u32 INFO = RecGeom<NW>::INFO, KBITS = 2 * KB + 6;
    const u32 info = base[INFO];
    const u32 j = i < ninst ? i - (info & 0x3ffu) : 0;
    const u32 n = (info >> 10) & 0xffu;
    const u32 s = 2 * (n - 1 - j);
    const u32* wp = base + (s >> 5);
    const u32 sh = s & 31;
    const u32 w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3], w4 = wp[4];
    u32 k0 = __builtin_amdgcn_alignbit(w1, w0, sh), k1 = __builtin_amdgcn_alignbit(w2, w1, sh);
    u32 k2 = __builtin_amdgcn_alignbit(w3, w2, sh), k3 = __builtin_amdgcn_alignbit(w4, w3, sh);
    k0 = (k0 & ~0x3fu) | (((info >> 18) & 0xffu) + j);  // idx' = idx0' + j (SuperKmerLight.hpp:98)
    // keep the 2kb + 6 key bits, put the routing id's low bits on top
    constexpr u32 m0 = KBITS >= 32 ? ~0u : (1u << KBITS) - 1, m1 = KBITS >= 64 ? ~0u : KBITS <= 32 ? 0u : (1u << (KBITS - 32)) - 1;
    constexpr u32 m2 = KBITS >= 96 ? ~0u : KBITS <= 64 ? 0u : (1u << (KBITS - 64)) - 1, m3 = KBITS >= 128 ? ~0u : KBITS <= 96 ? 0u : (1u << (KBITS - 96)) - 1;
    k0 &= m0; k1 &= m1; k2 &= m2; k3 &= m3;
    u64 lo = ((u64)k1 << 32) | k0, hi = ((u64)k3 << 32) | k2;
    if (SHIFT) {
        const u64 rl = (info >> 26) & ((1u << SHIFT) - 1);
        if (KBITS >= 64) hi |= rl << (KBITS - 64);
        else {
            lo |= rl << KBITS;
            if (KBITS + SHIFT > 64) hi |= rl >> (64 - KBITS);
        }
    }
    *lo_out = lo;
    *hi_out = hi;
}
// The table-free sibling of expand_and_dedupe_words (k_insert_first, finding 19): the partition's instances are known to be
// distinct, so every one of them is a new entry.  Keys only: no hash, nothing stored to LDS; li.won = the lane's slots in use.
template <u32 NI, u32 NW, u32 KB, u32 SHIFT, u32 NIMAX>
__device__ __forceinline__ void expand_words_distinct(u32 lane, u32 ninst, const u32* s_rw, const uint8_t* s_irec, LaneInst<NIMAX>& li) {
    static_assert(NI <= NIMAX, "instances per lane");
    u32 rix[NI];
    u32 won = 0;
#pragma unroll
    for (u32 it = 0; it < NI; it++) {
        const u32 i = it * 64 + lane;
        rix[it] = s_irec[i < ninst ? i : 0];
    }
#pragma unroll
    for (u32 it = 0; it < NI; it++) {
        const u32 i = it * 64 + lane;
        cut_key<NW, KB, SHIFT>(s_rw + rix[it] * RecGeom<NW>::RS, i, ninst, &li.klo[it], &li.khi[it]);
        if (i < ninst) won |= 1u << it;
    }
    li.won = won;
}
// s_imult: every instance slot's multiplicity, mod 256 (SAT: clamped to 255; the chunk's records folded: section 4 finding 15)
// (FOLD false: s_rmult, per record)
template <u32 NI, u32 NW, u32 KB, u32 SHIFT, u32 NIMAX, bool FOLD, bool SAT>
__device__ __forceinline__ void expand_and_dedupe_words(u32 lane, u32 ninst, u32 tsize, const u32* s_rw, const uint8_t* s_irec, const uint8_t* s_imult,
                                                        const u32* s_rmult, u64* s_key, u32* s_tab, u32* dbg_rounds, LaneInst<NIMAX>& li) {
    constexpr u32 RS = RecGeom<NW>::RS, KBITS = 2 * KB + 6;
    static_assert(KBITS + SHIFT <= 128 && SHIFT <= 6, "entry key: [routing id low bits | compacted k-mer | idx']");
    static_assert(NI <= NIMAX, "instances per lane");
    u64 (&klo)[NIMAX] = li.klo;
    u64 (&khi)[NIMAX] = li.khi;
    u32 (&hh)[NIMAX] = li.hh;
    u32 mult[NI];
    u32 rix[NI];
    u32 won = 0;
#pragma unroll
    for (u32 it = 0; it < NI; it++) {
        const u32 i = it * 64 + lane;
        rix[it] = s_irec[i < ninst ? i : 0];
    }
#pragma unroll
    for (u32 it = 0; it < NI; it++) {
        const u32 i = it * 64 + lane;
        u64 lo, hi;
        cut_key<NW, KB, SHIFT>(s_rw + rix[it] * RS, i, ninst, &lo, &hi);
        klo[it] = lo;
        khi[it] = hi;
        hh[it] = hash_key32(mk128(lo, hi)) & (tsize - 1);
        // counts wrap at 256 (SAT: stop at 255): so may the multiplicities
        mult[it] = FOLD ? (u32)s_imult[i < ninst ? i : 0] << WI_CNT_SHIFT : count8<SAT>(s_rmult[rix[it]]) << WI_CNT_SHIFT;
        if (i < ninst) {
            s_key[2 * i] = lo;
            s_key[2 * i + 1] = hi;
        }
    }
    wave_sync();  // every lane has read its records: the table may take their place
    for (u32 w = 0; w * 64 < tsize; w++) s_tab[w * 64 + lane] = EMPTY_SLOT;
    wave_sync();
    u32 pending = 0;
#pragma unroll
    for (u32 it = 0; it < NI; it++)
        if (it * 64 + lane < ninst) pending |= 1u << it;
    while (__any(pending != 0)) {
        *dbg_rounds += NI;
        u32 old[NI];
#pragma unroll
        for (u32 it = 0; it < NI; it++) {
            old[it] = EMPTY_SLOT;
            if (pending >> it & 1) old[it] = atomicCAS(&s_tab[hh[it]], EMPTY_SLOT, (it * 64 + lane) | mult[it]);
        }
        u64 olo[NI], ohi[NI];
#pragma unroll
        for (u32 it = 0; it < NI; it++) {
            const u32 oi = old[it] == EMPTY_SLOT ? 0 : (old[it] & WI_IDX_MASK);
            olo[it] = s_key[2 * oi];
            ohi[it] = s_key[2 * oi + 1];
        }
#pragma unroll
        for (u32 it = 0; it < NI; it++) {
            if (pending >> it & 1) {
                if (old[it] == EMPTY_SLOT) {
                    pending &= ~(1u << it);
                    won |= 1u << it;
                } else if (olo[it] == klo[it] && ohi[it] == khi[it]) {
                    atomicAdd(&s_tab[hh[it]], mult[it]);
                    pending &= ~(1u << it);
                } else {
                    hh[it] = (hh[it] + 1) & (tsize - 1);
                }
            }
        }
    }
    li.won = won;
}

// Record-level de-duplication of the <= 64 records the lanes hold (also in s_rec): the first copy of every distinct record
// survives, s_rmult[its lane] = the multiplicities of all its copies added up; returns whether this lane's record is a
// later copy.  Header bits 48..55 carry a record's multiplicity (mod 256: counts wrap there anyway; clamped to 255 in a saturating
// index) once a partition's records have been collapsed; they are not part of its identity.
#define HDR_ID_MASK 0x0000ffffffffffffull
#define HDR_HAS_MULT (1ull << 56)   // header bits 48..55 hold the record's multiplicity (a count byte: mod 256, or clamped to 255, as the index's counts are)
__device__ __forceinline__ bool dedupe_records(u32 stride, const RecRegs& rr, u32 my_mult, u32 nrec, u32 lane, const u64* s_rec, u32* s_rtab, u32* s_rmult) {
    s_rtab[lane] = EMPTY_SLOT;
    s_rtab[lane + 64] = EMPTY_SLOT;
    s_rmult[lane] = my_mult;
    wave_sync();
    bool dup = false;
    if (lane < nrec) {
        const u64 k1 = stride == 2 ? HDR_ID_MASK : ~0ull, k2 = stride == 3 ? HDR_ID_MASK : ~0ull, k3 = stride == 4 ? HDR_ID_MASK : ~0ull,
                  k4 = stride == 5 ? HDR_ID_MASK : ~0ull;
        const u64 w1 = rr.w1 & k1, w2 = rr.w2 & k2, w3 = rr.w3 & k3, w4 = rr.w4 & k4;
        // a weak hash is enough for <= 64 records in 128 slots: rotate-xor fold, one 32-bit multiply
        const u64 z = rr.w0 ^ ((w1 << 17) | (w1 >> 47)) ^ ((w2 << 31) | (w2 >> 33)) ^ ((w3 << 47) | (w3 >> 17)) ^ w4;
        u32 h = ((((u32)z ^ (u32)(z >> 32)) * 0x9E3779B1u) >> 20) & (2 * WI_MAX_REC - 1);
        for (;;) {
            const u32 o = atomicCAS(&s_rtab[h], EMPTY_SLOT, lane);
            if (o == EMPTY_SLOT) break;
            const u64* oc = s_rec + o * stride;
            bool same = oc[0] == rr.w0 && (oc[1] & k1) == w1;
            if (stride > 2) same = same && (oc[2] & k2) == w2;
            if (stride > 3) same = same && (oc[3] & k3) == w3;
            if (stride > 4) same = same && (oc[4] & k4) == w4;
            if (same) {
                atomicAdd(&s_rmult[o], my_mult);
                dup = true;
                break;
            }
            h = (h + 1) & (2 * WI_MAX_REC - 1);
        }
    }
    return dup;
}

// ---- Containment fold of a chunk's records (insert_body's FOLD bodies, DESIGN.md section 4 finding 15).  Record B is contained
// in record A when their routing ids are equal, A's idx' range holds B's and B's compacted string is the matching part of
// A's: then every key of B is the key of A with the same idx', bit for bit, whatever the data.  A contained record is not
// expanded; its k-mers' multiplicity is added over the range of its leader's instance slots.  The strings are compared in a
// frame common to all records: the k-mer of idx' t starts at nucleotide E - 1 - t (E = suff_reduc + k - m + 1 bounds every
// record's idx0' + n), so record R's string sits shifted left by 2(E - idx0'_R - n_R) bits, and "B in A" is
// (U_A & M_B) == U_B with M_B the ones over B's nucleotides -- no shift per pair.  The frame is 2k - m - b nucleotides wide:
// it fits the record's words.
#ifndef WI_FOLD_TRIPS
#define WI_FOLD_TRIPS 16u   // heads per chunk at most (a wave-wide round each); records still open after them stay unfolded
#endif
struct FoldFrame {
    W4 u, m;    // the record's string in the common frame, and the ones over its nucleotides (NW words used)
    u32 rid;    // routing id
    u32 rng;    // idx0' | (idx0' + n) << 8
    u32 s;      // (n << 6) | (63 - lane): the order heads are taken in (0: the record takes no part)
};
template <u32 NW, u32 KB>
__device__ __forceinline__ FoldFrame fold_frame(const RecRegs& rr, u64 hdr, u32 n, bool valid, u32 frame_end, u32 lane) {
    FoldFrame f;
    const u32 idx0 = hdr_idx0(hdr), end = idx0 + n, top = frame_end - idx0 + KB - 1;  // nucleotides below the string's top
    // (a record outside the frame -- none the scan emits -- takes no part: it is expanded on its own)
    const bool ok = valid && n > 0 && end <= frame_end && top <= 32 * NW;
    const u32 lo_bits = ok ? 2 * (frame_end - end) : 0, hi_bits = ok ? 2 * top : 0;
    f.m = w4_andn(w4_mask(hi_bits), w4_mask(lo_bits));
    f.u = w4_and(w4_shl(W4{rr.w0, NW > 1 ? rr.w1 : 0, NW > 2 ? rr.w2 : 0, NW > 3 ? rr.w3 : 0}, lo_bits), f.m);
    f.rid = hdr_bucket(hdr);
    f.rng = idx0 | (end << 8);
    f.s = ok ? (n << 6) | (63 - lane) : 0;
    return f;
}
__device__ __forceinline__ u64 readlane64(u64 v, u32 a) {
    return ((u64)(u32)__builtin_amdgcn_readlane((int)(v >> 32), (int)a) << 32) | (u32)__builtin_amdgcn_readlane((int)v, (int)a);
}
// Folds the records of lanes < nrec.  Heads are taken in decreasing (n, -lane) among the records still open, one wave-wide
// round each: the head is maximal (a record containing it would be larger, and open: what contains a folded record contains
// its head too), and every open record it contains folds into it.  Returns whether this lane's record folded; *lead: the
// lane of its head (its own lane otherwise), *off: its idx0' minus the head's.  Identical records fold into the lowest lane
// of them, so no separate record-level de-duplication is needed.
//
// DETECT (k_insert_first, section 4 finding 19): *clean comes back true only where the rounds PROVE that no two k-mer instances
// of the surviving records have equal keys.  Two records can share a key only if their routing ids are equal, their idx'
// ranges intersect and their strings agree on a whole window of the intersection; every window of an idx' in
// [suff_reduc, suff_reduc + w] covers the frame's nucleotides [w, k - b) (the core: fold_core), so records that differ there
// share none.  The caller hands every record's `ck`, [routing id low bits | core] -- a partition's records differ in nothing
// else of the routing id -- so "same routing id and core" is one 32-bit compare.  In the round of head A every record still
// open after the containment test whose ck is A's and whose range meets A's clears *clean; so does a record still open after
// the last round (those were never compared with each other), and one `unsure` on entry (outside the frame, or below
// suff_reduc: the caller says).  Why that is enough: every pair of survivors was compared in the round in which the earlier of
// the two was head (the later one was open then: a survivor closes only as a head), a folded record adds no instances, and
// within one record the idx' differ.  The cost per round is one v_readlane and the compare; the lanes' findings add up in one
// register, and one test after the rounds reads it.
template <u32 KB, u32 CW>
__device__ __forceinline__ u32 fold_core(const W4& u) {  // the frame bits [2 CW, 2 KB) every k-mer window covers (CW = k - m, KB = k - b)
    constexpr u32 LO = 2 * CW, N = 2 * (KB - CW), WI = LO / 64, BI = LO % 64;
    static_assert(CW < KB && N <= 28 && LO + N <= 256, "the core: the minimizer's nucleotides that are not cut out, m - b of them");
    const u64 w[5] = {u.w0, u.w1, u.w2, u.w3, 0};
    u64 v = w[WI] >> BI;
    if (BI + N > 64) v |= w[WI + 1] << (64 - BI);
    return (u32)v & ((1u << N) - 1);
}
template <u32 NW, bool DETECT = false>
__device__ __forceinline__ bool fold_records(const FoldFrame& f, u32 nrec, u32 lane, u32* lead, u32* off, u32* trips, u32 ck = 0, bool unsure = false, bool* clean = nullptr) {
    u32 sv = lane < nrec ? f.s : 0;
    bool folded = false;
    u32 dirty = unsure;
    *lead = lane;
    *off = 0;
    for (u32 t = 0; t < WI_FOLD_TRIPS; t++) {
        const u32 smax = (u32)__builtin_amdgcn_readlane((int)wave_incl_max_scan(sv), 63);
        if (smax == 0) break;
        *trips += 1;
        const u32 a = 63 - (smax & 63);
        const u32 rid_a = (u32)__builtin_amdgcn_readlane((int)f.rid, (int)a), rng_a = (u32)__builtin_amdgcn_readlane((int)f.rng, (int)a);
        const u32 i0 = f.rng & 0xffu, e = f.rng >> 8, i0a = rng_a & 0xffu, ea = rng_a >> 8;
#ifdef BRISK_NO_RECORD_FOLD  // A/B: identical records only (what the record-level de-duplication collapsed)
        bool in = sv != 0 && rid_a == f.rid && i0a == i0 && ea == e;
#else
        bool in = sv != 0 && rid_a == f.rid && i0a <= i0 && e <= ea;
#endif
        bool same = (readlane64(f.u.w0, a) & f.m.w0) == f.u.w0;
        if (NW > 1) same = same & ((readlane64(f.u.w1, a) & f.m.w1) == f.u.w1);
        if (NW > 2) same = same & ((readlane64(f.u.w2, a) & f.m.w2) == f.u.w2);
        if (NW > 3) same = same & ((readlane64(f.u.w3, a) & f.m.w3) == f.u.w3);
        in = in && same;
        if (in) {  // (the head itself closes here, unfolded)
            sv = 0;
            if (lane != a) {
                folded = true;
                *lead = a;
                *off = i0 - i0a;
            }
        }
        if (DETECT) {  // (what is still open is neither the head nor contained in it)
            const u32 differs = ck ^ (u32)__builtin_amdgcn_readlane((int)ck, (int)a);
            const u32 meets = ((i0 - ea) & (i0a - e)) >> 31;  // 1: i0 < ea && i0a < e (all below 256)
            dirty |= (differs == 0 && sv != 0) ? meets : 0u;
        }
    }
    if (DETECT) *clean = !__any((dirty | sv) != 0);
    return folded;
}

// ---- The same fold with the head of every core-key group taken in the same round (k_insert_first, section 4 finding 21).  Where
// no record is `unsure`, every record's mask covers the core, so a record is contained only in a head of its own ck and makes
// only records of its own ck dirty: the groups' rounds do not interact, and a partition of four loci need not spend four
// wave-wide rounds on them.  A lane's slot is a 6-bit hash of its ck (fold_slot).  A round: the open lanes ds_max their
// [round | sv] into their slot of `s_slot` (64 words, cleared once: a later round's values lie above every earlier one's), read
// the slot back, and meet the head they find there -- its rng, ck and frame words fetched by lane index (ds_bpermute), a word at
// a time, where fold_records broadcasts them through scalar registers.  The lane whose own value came back is a head and closes
// unfolded.  Two groups in one slot cost rounds, not correctness: the smaller head's group fails the ck compare, stays open and
// finds its own head in a later round; within a group heads are still taken in decreasing sv, so lead, off, folded and clean
// are fold_records' wherever that takes at most WI_FOLD_TRIPS heads.  Returns false -- nothing of the result is to be used, the
// caller runs fold_records -- where a record is unsure (containment then need not imply equal ck), where more heads than that
// were taken, or where a lane is open after the last round.
// Two partitions in one wave (finding 22) are just more groups: the caller sets a partition bit in B's ck, so a record meets
// only heads of its own partition; *dirty_lanes is the ballot of the lanes found dirty, which the caller reduces per partition.
#ifndef FOLD_GROUPED
#define FOLD_GROUPED 1   // -DFOLD_GROUPED=0: fold_records alone in k_insert_first, for A/B
#endif
#ifdef INSERT_ATTR_ONEROUND  // attribution build: the fold stops after one round.  Wrong results, timing only
#define FOLD_GROUPED_TRIPS 1u
#else
#define FOLD_GROUPED_TRIPS WI_FOLD_TRIPS
#endif
__device__ __forceinline__ u32 fold_slot(u32 ck) { return (ck * 0x9E3779B1u) >> 26; }
__device__ __forceinline__ u32 lane_fetch(u32 v, u32 a4) { return (u32)__builtin_amdgcn_ds_bpermute((int)a4, (int)v); }
__device__ __forceinline__ u64 lane_fetch64(u64 v, u32 a4) { return ((u64)lane_fetch((u32)(v >> 32), a4) << 32) | lane_fetch((u32)v, a4); }
template <u32 NW>
__device__ __forceinline__ bool fold_records_grouped(const FoldFrame& f, u32 nrec, u32 lane, u32* s_slot, u32* lead, u32* off, bool* folded_out, u32* trips, u32 ck, bool unsure,
                                                     bool* clean, unsigned long long* dirty_lanes = nullptr) {
    static_assert(WI_FOLD_TRIPS < (1u << 18), "[round | n | 63 - lane] in 32 bits: n < 256, so sv < 1 << 14");
    if (__any(unsure)) return false;
    u32 sv = lane < nrec ? f.s : 0;
    bool folded = false;
    u32 dirty = 0, heads = 0;
    *lead = lane;
    *off = 0;
    u32* my_slot = s_slot + fold_slot(ck);
    s_slot[lane] = 0;
    wave_sync();
    for (u32 t = 1; t <= FOLD_GROUPED_TRIPS; t++) {
        if (!__any(sv != 0) || heads > WI_FOLD_TRIPS) break;
        *trips += 1;
        const u32 mine = (t << 14) | sv;
        if (sv != 0) atomicMax(my_slot, mine);
        wave_sync();
        const u32 top = *my_slot;  // (a closed lane reads what it likes: every use below is under sv != 0)
        heads += (u32)__popcll(__ballot(sv != 0 && top == mine));
        const u32 a = 63 - (top & 63), a4 = a << 2;
        const u32 rng_a = lane_fetch(f.rng, a4), ck_a = lane_fetch(ck, a4);
        const u32 i0 = f.rng & 0xffu, e = f.rng >> 8, i0a = rng_a & 0xffu, ea = rng_a >> 8;
        bool in = sv != 0 && ck_a == ck && i0a <= i0 && e <= ea;  // (equal ck: equal routing ids, a partition's differ in nothing else)
        bool same = (lane_fetch64(f.u.w0, a4) & f.m.w0) == f.u.w0;
        if (NW > 1) same = same & ((lane_fetch64(f.u.w1, a4) & f.m.w1) == f.u.w1);
        if (NW > 2) same = same & ((lane_fetch64(f.u.w2, a4) & f.m.w2) == f.u.w2);
        if (NW > 3) same = same & ((lane_fetch64(f.u.w3, a4) & f.m.w3) == f.u.w3);
        in = in && same;
        if (in) {  // (a head closes here, unfolded)
            sv = 0;
            if (lane != a) {
                folded = true;
                *lead = a;
                *off = i0 - i0a;
            }
        }
        const u32 meets = ((i0 - ea) & (i0a - e)) >> 31;  // 1: i0 < ea && i0a < e (all below 256)
        dirty |= (ck_a == ck && sv != 0) ? meets : 0u;
    }
#ifndef INSERT_ATTR_ONEROUND
    if (heads > WI_FOLD_TRIPS || __any(sv != 0)) return false;
#endif
    const unsigned long long dl = __ballot(dirty != 0);  // (a lane is made dirty only by a head of its own ck: of its own partition, where two share the wave)
    if (dirty_lanes) *dirty_lanes = dl;
    *clean = dl == 0;
    *folded_out = folded;
    return true;
}

// MAXI: k-mer instances per chunk.  256 (10 KB of LDS, 128 registers: 4 waves per SIMD) for the usual partitions of a
// few hundred instances; 512 (2 waves per SIMD) when partitions are big -- few distinct minimizers, as with m <= 11 --
// and the passes over a partition's entries saved by half as many chunks outweigh the occupancy.
// NW > 0: the record width (u64 words of the compacted super-k-mer), kb = k - b and the routing-id bits kept in the
// key are compile-time constants (the common parameter sets; the host picks the instantiation): shifts, masks and
// strides fold, nothing of BriskParams stays in scalar registers (the generic body spills 48 of them into vector
// lanes and pays a v_readlane per use), and k-mers are cut out of 32-bit words (expand_and_dedupe_words).  NW == 0:
// everything from P at run time.
// SAT: the index's counts stop at 255 instead of wrapping (count8).
// LISTED: the wave walks desc[list[0 .. *n_list)] instead of desc[0 .. n_touched): the partitions k_insert_first left over.  The
// count is read from device memory, so the host need not wait for it.  A compile-time switch: the unlisted bodies are
// instruction for instruction what they were.
template <u32 MAXI, u32 NW, u32 KB, u32 SHIFT, bool SAT, bool LISTED = false>
__device__ __forceinline__ void insert_body(const BriskParams& PP, const RecSrc& src, const PartDesc* __restrict__ desc, u32 n_touched_all, const IndexDev& ix,
                                            u32* __restrict__ work_counter, const u32* __restrict__ list = nullptr, const u32* __restrict__ n_list = nullptr) {
    const u32 n_touched = LISTED ? min(*n_list, n_touched_all) : n_touched_all;
    u64* const rec = src.rec;  // the in-place collapse of the big-partition kernel (classic layout only)
    BriskParams P = PP;
    if (NW) {  // the fields the body reads, as constants
        P.nw = NW;
        P.stride = NW + 1;
        P.kb = KB;
        P.shift = SHIFT;
    }
    constexpr u32 TABLE = 2 * MAXI, TS = TABLE / 64, NI = MAXI / 64;
    constexpr u32 KW = NW ? (2 * KB + 6 + SHIFT <= 64 ? 1u : 2u) : 0u;  // words of a stored key (0: ix.key_words)
    // The containment fold (fold_records) where it measured faster: k63 (three record words) in chunks of 256 instances.
    // At k31 (k31 m15 b14, k31 m11 b11 in the 512-instance body) its rounds cost more than the instances they save.
    constexpr bool FOLD = NW >= 3 && MAXI == WI_MAX_INST;
    static_assert(MAXI % 256 == 0 && MAXI <= 1024, "chunk size: whole 32-bit words of record marks per lane, 10-bit instance index");
    // LDS of one wave, one buffer cut into regions.  k_insert's throughput follows the number of resident waves almost
    // linearly (4096 -> 30.8 ms, 3072 -> 38.3, 2048 -> 54.2, 1024 -> 103.6 per 50 M reads: every wave is a serial chain of
    // LDS and memory round trips), so what is not live at the same time shares its bytes.  Compile-time geometry (NW > 0):
    // the probe table lies over the records' region -- the records are last read when the keys are built, the table is
    // first written right after -- and nothing of the generic body's prefix array exists: 7,680 B per wave instead of
    // 10,000, i.e. 21 waves per CU by LDS instead of 16.
    //   s_key   [2 * MAXI] u64   the instances' keys                          expand .. stream
    //   s_rec   [REC_U64]  u64   records as u64 words (record-level pass), then as shifted 32-bit words (s_rw; + 4 words:
    //                            the last record's window reads two words past its slot), generic: then the new entries' list
    //   s_tab   [TABLE]    u32   probe table                                   NW > 0: over s_rec
    //   s_rtab, s_rmult, s_irec, (generic: s_pref)
    constexpr u32 REC_U64 = WI_MAX_REC * 5 > MAXI / 2 ? WI_MAX_REC * 5 : MAXI / 2;
    static_assert(NW == 0 || (WI_MAX_REC * RecGeom<NW ? NW : 1>::RS + 4) * 4 <= REC_U64 * 8, "shifted record words must fit the record buffer");
    constexpr bool TAB_OVER_REC = NW && TABLE * 4 <= REC_U64 * 8;  // (the 512-instance body's table is larger than its record buffer)
    constexpr u32 OFF_REC = 16 * MAXI, OFF_TAB = TAB_OVER_REC ? OFF_REC : OFF_REC + 8 * REC_U64, OFF_RTAB = TAB_OVER_REC ? OFF_REC + 8 * REC_U64 : OFF_TAB + 4 * TABLE;
    constexpr u32 OFF_RMULT = OFF_RTAB + 4 * 2 * WI_MAX_REC, OFF_IREC = OFF_RMULT + 4 * WI_MAX_REC, OFF_PREF = OFF_IREC + MAXI;
    constexpr u32 LDS_BYTES = NW ? OFF_PREF : OFF_PREF + 4 * (WI_MAX_REC + 1) + 4;
    __shared__ __attribute__((aligned(16))) unsigned char s_mem[LDS_BYTES];
    u64* s_key = (u64*)s_mem;
    u32* s_idiff = (u32*)s_mem;  // FOLD: [MAXI] the instances' multiplicity steps, over the first quarter of s_key (instance map)
    u64* s_rec = (u64*)(s_mem + OFF_REC);
    u32* s_rw = (u32*)s_rec;
    u32* s_tab = (u32*)(s_mem + OFF_TAB);
    u32* s_list = (u32*)s_rec;  // generic body: [MAXI] the new entries' table words, built after the records have been expanded
    u32* s_rtab = (u32*)(s_mem + OFF_RTAB);
    u32* s_rmult = (u32*)(s_mem + OFF_RMULT);
    uint8_t* s_irec = s_mem + OFF_IREC;
    uint8_t* s_imult = s_mem + OFF_RTAB;  // FOLD: [MAXI] the instances' multiplicities mod 256 (instance map .. expand), over s_rtab
    static_assert(NW == 0 || MAXI <= 4 * 2 * WI_MAX_REC, "instance multiplicities fit the record table's bytes");
    u32* s_pref = (u32*)(s_mem + (NW ? 0 : OFF_PREF));  // generic body only

    const u32 lane = threadIdx.x;
    PHASE_DECL
    unsigned long long acur = ix.slot_cur[blockIdx.x], aend = ix.slot_end[blockIdx.x], garbage = 0;
    const u32 kbits = 2 * P.kb + 6;

    for (;;) {
        // ---- take the next batch of partitions (one atomic per WI_BATCH partitions)
        u32 t0 = 0;
        if (lane == 0) t0 = atomicAdd(work_counter, WI_BATCH);
        t0 = (u32)__builtin_amdgcn_readfirstlane((int)t0);
        if (t0 >= n_touched) break;
        const u32 t_end = min(t0 + WI_BATCH, n_touched);
        // A partition's descriptor comes by scalar loads (s_load_dwordx8: t and the array's address are wave-uniform, the array is
        // read-only).  Round 2 kept the batch's 64 descriptors in registers, one per lane, and broadcast one with eight v_readlane:
        // those were the eight registers the body spilled at 96 (10 spilled -> 3; 26.2 -> 25.9 ms per 50 M reads).
        PartDesc d = desc[LISTED ? list[t0] : t0];
        RecRegs rr = load_part_recs(P, src, d.part, d.r_begin, d.r_begin, min(d.n_rec, (u32)WI_MAX_REC), lane);

        for (u32 t = t0; t < t_end; t++) {
            const u32 tn = t + 1;
            PartDesc dn{};
            if (tn < t_end) dn = desc[LISTED ? list[tn] : tn];
            // The next partition's records are requested when this partition is done, into rr.  Round 2 requested them at the top
            // of the current partition, into a second set of registers: the memory counter retires loads in issue order and the
            // compiler's wait in front of the first use of rr is vmcnt(0), so every partition began by sitting out the round trip
            // of the prefetch it had just issued, and kept eight more registers live for it (31.1 ms per 50 M reads against 30.0
            // this way; requesting them in front of the partition's last stores, or where the last chunk has expanded its
            // records, measured 32.6 / 32.3: DESIGN.md section 4).
#define NEXT_PARTITION                                                                                                  \
    {                                                                                                                   \
        d = dn;                                                                                                         \
        if (tn < t_end) rr = load_part_recs(P, src, d.part, d.r_begin, d.r_begin, min(d.n_rec, (u32)WI_MAX_REC), lane); \
    }

            // rr must have landed on EVERY path before it is requested again at the end of the partition (a load's destination
            // is not written while the load is in flight), a partition left to k_insert_huge or one whose lanes all skip the
            // store below included: without this unconditional use the compiler waits at the end of every partition instead --
            // for all the stores the partition has just issued.
            asm volatile("" ::"v"(rr.w0), "v"(rr.w1), "v"(rr.w2), "v"(rr.w3), "v"(rr.w4));
            do {  // (one pass: a partition that is not this kernel's leaves through `break`)
            if (ix.huge_at && d.n_inst > ix.huge_at) break;  // a block of 16 waves takes this one (k_insert_huge)
            CNT(0, 1)
            const u32 part = d.part;
            u32 r_end = d.r_begin + d.n_rec;
            u32 n_exist = d.n_exist;
            u32 inst_left = d.n_inst;  // instances not yet processed: bounds the final size
            unsigned long long off = d.off;
            u32 cap = d.cap;
            u32 bm0 = 0, bm1 = 0;

            // A partition of many records (one hot bucket) first collapses its records window by window, in place:
            // the chunks below then see each distinct record of a window once, with its multiplicity in the header,
            // and far fewer chunks -- each of which streams the partition's entries -- are needed.
            // (only in the big-partition kernel: the usual one is 2-3 % slower with this path compiled in)
            bool collapsed = false;
            if (MAXI > WI_MAX_INST && !src.bin_cap && d.n_rec > 2 * WI_MAX_REC) {
                u32 wr = d.r_begin;
                for (u32 rd = d.r_begin; rd < r_end; rd += WI_MAX_REC) {
                    const u32 avail = min(r_end - rd, (u32)WI_MAX_REC);
                    if (rd != d.r_begin) rr = load_rec_regs(P, rec, rd, avail, lane);
                    wave_sync();
                    if (lane < avail) {
                        u64* dst = s_rec + lane * P.stride;
                        dst[0] = rr.w0;
                        dst[1] = rr.w1;
                        if (P.stride > 2) dst[2] = rr.w2;
                        if (P.stride > 3) dst[3] = rr.w3;
                        if (P.stride > 4) dst[4] = rr.w4;
                    }
                    // a record may carry a multiplicity already (brisk_hip_reallocate: one k-mer with its entry's count): it is what
                    // the record adds to its survivor, and it is replaced, not OR-ed over, in the survivor's header
                    const u64 hdr_c = P.stride == 2 ? rr.w1 : P.stride == 3 ? rr.w2 : P.stride == 4 ? rr.w3 : rr.w4;
                    const u32 mult_c = (hdr_c & HDR_HAS_MULT) ? (u32)(hdr_c >> 48) & 0xffu : 1u;
                    const bool dup = dedupe_records(P.stride, rr, mult_c, avail, lane, s_rec, s_rtab, s_rmult);
                    wave_sync();
                    const bool keep = lane < avail && !dup;
                    const unsigned long long bal = __ballot(keep);
                    if (keep) {  // survivors move to the front of the partition's records (never past what is still to be read)
                        u64* dst = rec + (u64)(wr + (u32)__popcll(bal & lanes_below(lane))) * P.stride;
                        const u64 keep_id = HDR_ID_MASK, mult = ((u64)count8<SAT>(s_rmult[lane]) << 48) | HDR_HAS_MULT;  // (a window's copies add up to 64 x 255 at most)
                        dst[0] = rr.w0;
                        dst[1] = P.stride == 2 ? (rr.w1 & keep_id) | mult : rr.w1;
                        if (P.stride > 2) dst[2] = P.stride == 3 ? (rr.w2 & keep_id) | mult : rr.w2;
                        if (P.stride > 3) dst[3] = P.stride == 4 ? (rr.w3 & keep_id) | mult : rr.w3;
                        if (P.stride > 4) dst[4] = (rr.w4 & keep_id) | mult;
                    }
                    wr += (u32)__popcll(bal);
                }
                collapsed = true;
                r_end = wr;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the chunks read what was just written: same wave, same CU
                rr = load_rec_regs(P, rec, d.r_begin, min(r_end - d.r_begin, (u32)WI_MAX_REC), lane);
            }

            for (u32 rc = d.r_begin; rc < r_end;) {
                // ---- pick the chunk: up to WI_MAX_REC records / MAXI instances
                PHASE(0)
                CNT(1, 1)
                const u32 avail = min(r_end - rc, (u32)WI_MAX_REC);
                if (rc != d.r_begin) rr = load_part_recs(P, src, part, d.r_begin, rc, avail, lane);
                wave_sync();
                if (!FOLD && lane < avail) {  // (the record-level pass reads them here; the fold works from registers)
                    u64* dst = s_rec + lane * P.stride;
                    dst[0] = rr.w0;
                    dst[1] = rr.w1;
                    if (P.stride > 2) dst[2] = rr.w2;
                    if (P.stride > 3) dst[3] = rr.w3;
                    if (P.stride > 4) dst[4] = rr.w4;
                }
                const u64 my_hdr = P.stride == 2 ? rr.w1 : P.stride == 3 ? rr.w2 : P.stride == 4 ? rr.w3 : rr.w4;
                const u32 raw_n = lane < avail ? hdr_n(my_hdr) : 0;
                // a record stands for one vector, unless its header says how many (collapsed records above; the entries of
                // an index being re-bucketed, brisk_hip_reallocate: one k-mer with its count)
                const u32 my_mult = (my_hdr & HDR_HAS_MULT) ? (u32)(my_hdr >> 48) & 0xffu : 1u;
                const u32 x0 = wave_incl_scan(raw_n, lane);
                // First try every available record: identical records (the same super-k-mer seen in
                // several reads) collapse into one with a multiplicity, so far more raw instances fit.
                // If the collapsed chunk is still too big, shrink to the prefix whose collapsed count fits (counted
                // again on its own it can come out a little higher, once the first copy of a record lies beyond
                // it: hence the loop), at the latest to the raw-count prefix, which always fits.
                const u32 rawfit = (u32)__popcll(__ballot(lane < avail && x0 <= MAXI));  // >= 1; a prefix: x0 is monotone
                u32 nrec = avail, my_n = 0, x = 0, ninst = 0;
                // FOLD: records contained in others (identical ones included) fold into them instead (fold_records):
                // 185 -> ~85 instances per partition at k63 m21 b14 (section 4 finding 15).
                u32 lead = lane, lead_off = 0, dbg_trips = 0;
                FoldFrame ff{};
                // FOLD: the records as 32-bit words of C << 6 (expand_and_dedupe_words) right away, their info words once the
                // prefix is known: the record registers are dead from here on
                const u32 info_hi = (raw_n << 10) | (hdr_idx0(my_hdr) << 18) | ((hdr_bucket(my_hdr) & ((1u << SHIFT) - 1)) << 26);
                if (FOLD) {
                    ff = fold_frame<NW ? NW : 1, KB>(rr, my_hdr, raw_n, lane < avail, P.suff_reduc + P.w + 1, lane);
                    if (lane < avail) store_rec_words<NW ? NW : 1>(s_rw + lane * RecGeom<NW ? NW : 1>::RS, rr, 0);
                }
                for (int attempt = 0;; attempt++) {
                    CNT(2, 1)
                    bool dup;
                    if (FOLD) dup = fold_records<NW ? NW : 1>(ff, nrec, lane, &lead, &lead_off, &dbg_trips);
                    else dup = dedupe_records(P.stride, rr, my_mult, nrec, lane, s_rec, s_rtab, s_rmult);
                    my_n = (lane < nrec && !dup) ? raw_n : 0;
                    x = wave_incl_scan(my_n, lane);
                    ninst = __shfl(x, 63, 64);
                    if (ninst <= MAXI) break;
                    const u32 fit = (u32)__popcll(__ballot(lane < nrec && x <= MAXI));  // x is monotone too
                    nrec = (attempt >= 2 || fit <= rawfit) ? rawfit : min(fit, nrec - 1);
                    wave_sync();
                }
                PHASE(1)
                const u32 raw_inst = __shfl(x0, nrec - 1, 64);
                CNT(9, raw_inst)
                CNT(10, FOLD ? (u32)__popcll(__ballot(lane < nrec && my_n == 0 && raw_n != 0)) : 0u)
                CNT(11, dbg_trips)
                // (what k_insert_first would meet: a partition's instances after the fold, by slots of 64 per lane, and the
                // partitions of more records than one chunk holds)
                CNT(12, rc == d.r_begin && d.n_rec <= WI_MAX_REC && ninst > 64 && ninst <= 128 ? 1u : 0u)
                CNT(13, rc == d.r_begin && d.n_rec <= WI_MAX_REC && ninst > 128 && ninst <= 192 ? 1u : 0u)
                CNT(14, rc == d.r_begin && d.n_rec <= WI_MAX_REC && ninst > 192 ? 1u : 0u)
                CNT(15, rc == d.r_begin && d.n_rec > WI_MAX_REC ? 1u : 0u)
                // where this record's k-mers sit on the instance line: its own slots, or its head's from its idx0' on
                const u32 m_first = FOLD ? (u32)__shfl(x - my_n, lead, 64) + lead_off : 0u;
                // (a quarter full at most in instances, less in distinct keys: probe rounds are wave-wide -- every round costs all 64 lanes
                // whoever is still probing -- so a sparser table is worth its clearing: 25.8 -> 25.0 ms per 50 M reads against half full.
                // Skipping, by a scalar branch, the instance slots nobody is pending in lost: 28.7 ms -- seven more spilled registers)
                u32 tsize = 128;
                while (tsize < 4 * ninst && tsize < TABLE) tsize <<= 1;
                if (!NW) {  // (compile-time geometry: the prefix travels in the records' info words, and the table -- which lies
                            // over the records there -- is cleared once the keys have been built from them)
                    s_pref[lane + 1] = x;
                    if (lane == 0) s_pref[0] = 0;
#pragma unroll
                    for (u32 w = 0; w < TS; w++)
                        if (w * 64 < tsize) s_tab[w * 64 + lane] = EMPTY_SLOT;
                }
                {
                    // instance -> record: each record marks its first instance, a running maximum spreads the marks
                    // (records lie in lane order).  Every lane owns MAXI/64 consecutive instances here.
                    // FOLD, in the same rounds: every instance's multiplicity.  Each record adds its own
                    // at the start of its range and takes it off at the end; a prefix sum over the slots (the lane's NI,
                    // then the wave) adds up the records over every slot.  u32, wrapping: the steps cancel, so every slot's sum is exact
                    // (64 records x 255 at most) and its count byte is taken from it (count8).
                    u32* irec32 = (u32*)s_irec;
#pragma unroll
                    for (u32 q = 0; q < MAXI / 256; q++) irec32[q * 64 + lane] = 0;
                    if (FOLD) {
#pragma unroll
                        for (u32 q = 0; q < NI; q++) s_idiff[lane * NI + q] = 0;
                    }
                    wave_sync();
                    if (my_n) s_irec[x - my_n] = (uint8_t)(lane + 1);
                    if (FOLD && lane < nrec) {
                        atomicAdd(&s_idiff[m_first], my_mult);
                        if (m_first + raw_n < ninst) atomicAdd(&s_idiff[m_first + raw_n], 0u - my_mult);
                    }
                    wave_sync();
                    u32 wv[MAXI / 256], run = 0;
#pragma unroll
                    for (u32 q = 0; q < MAXI / 256; q++) {
                        wv[q] = irec32[lane * (MAXI / 256) + q];
                        run = op_max_u32(run, op_max_u32(op_max_u32(wv[q] & 0xff, (wv[q] >> 8) & 0xff), op_max_u32((wv[q] >> 16) & 0xff, wv[q] >> 24)));
                    }
                    if (FOLD) {
                        u32 mv[NI], tot = 0;
#pragma unroll
                        for (u32 q = 0; q < NI; q++) {
                            tot += s_idiff[lane * NI + q];
                            mv[q] = tot;
                        }
                        const u32 before = wave_incl_scan(tot, lane) - tot;
                        u32* mult32 = (u32*)s_imult;
#pragma unroll
                        for (u32 q = 0; q < NI / 4; q++)
                            mult32[lane * (NI / 4) + q] = count8<SAT>(mv[4 * q] + before) | (count8<SAT>(mv[4 * q + 1] + before) << 8) |
                                                          (count8<SAT>(mv[4 * q + 2] + before) << 16) |
                                                          ((SAT ? count8<SAT>(mv[4 * q + 3] + before) : mv[4 * q + 3] + before) << 24);
                    }
                    u32 carry = wave_prev_lane(wave_incl_max_scan(run));  // the last mark before this lane's instances
#pragma unroll
                    for (u32 q = 0; q < MAXI / 256; q++) {
                        const u32 b0 = op_max_u32(carry, wv[q] & 0xff), b1 = op_max_u32(b0, (wv[q] >> 8) & 0xff);
                        const u32 b2 = op_max_u32(b1, (wv[q] >> 16) & 0xff), b3 = op_max_u32(b2, wv[q] >> 24);
                        carry = b3;
                        // marks are lane + 1; instances past the last record (none are read) may hold 0 - 1
                        irec32[lane * (MAXI / 256) + q] = ((b0 - 1) & 0xff) | (((b1 - 1) & 0xff) << 8) | (((b2 - 1) & 0xff) << 16) | ((b3 - 1) << 24);
                    }
                }
                wave_sync();
                // ---- 0/1. expand to entry keys and de-duplicate
                PHASE(2)
                u32 dbg_r = 0;
                LaneInst<NI> li;
                li.won = 0;
                CNT(3, (ninst + 63) / 64)
                CNT(4, ninst)
                CNT(5, nrec)
                if (NW) {
                    // the records' info words: [first instance | n | idx0' | routing id low bits]
                    if (FOLD && lane < nrec) s_rw[lane * RecGeom<NW ? NW : 1>::RS + RecGeom<NW ? NW : 1>::INFO] = (x - my_n) | info_hi;
                    if (!FOLD && lane < nrec) store_rec_words<NW ? NW : 1>(s_rw + lane * RecGeom<NW ? NW : 1>::RS, rr, (x - my_n) | info_hi);
                    wave_sync();
                    if (ninst <= 64) expand_and_dedupe_words<1, NW ? NW : 1, KB, SHIFT, NI, FOLD, SAT>(lane, ninst, tsize, s_rw, s_irec, s_imult, s_rmult, s_key, s_tab, &dbg_r, li);
                    else if (ninst <= 128) expand_and_dedupe_words<2, NW ? NW : 1, KB, SHIFT, NI, FOLD, SAT>(lane, ninst, tsize, s_rw, s_irec, s_imult, s_rmult, s_key, s_tab, &dbg_r, li);
                    else if (ninst <= 192) expand_and_dedupe_words<3, NW ? NW : 1, KB, SHIFT, NI, FOLD, SAT>(lane, ninst, tsize, s_rw, s_irec, s_imult, s_rmult, s_key, s_tab, &dbg_r, li);
                    else if (NI <= 4 || ninst <= 256) expand_and_dedupe_words<4, NW ? NW : 1, KB, SHIFT, NI, FOLD, SAT>(lane, ninst, tsize, s_rw, s_irec, s_imult, s_rmult, s_key, s_tab, &dbg_r, li);
                    else expand_and_dedupe_words<NI, NW ? NW : 1, KB, SHIFT, NI, FOLD, SAT>(lane, ninst, tsize, s_rw, s_irec, s_imult, s_rmult, s_key, s_tab, &dbg_r, li);
                } else {
                    if (ninst <= 128) expand_and_dedupe<2, 0, SAT>(P, lane, ninst, tsize, s_rec, s_pref, s_irec, s_rmult, s_key, s_tab);
                    else if (NI <= 4 || ninst <= 256) expand_and_dedupe<4, 0, SAT>(P, lane, ninst, tsize, s_rec, s_pref, s_irec, s_rmult, s_key, s_tab);
                    else expand_and_dedupe<NI, 0, SAT>(P, lane, ninst, tsize, s_rec, s_pref, s_irec, s_rmult, s_key, s_tab);
                }
                wave_sync();
                CNT(8, dbg_r)
                PHASE(3)

                // ---- 2. existing entries probe the table.  After the first chunk they include what this wave
                // appended itself: same wave, same CU, so those stores only have to be complete (workgroup
                // scope; __threadfence() would write back and invalidate the XCD's whole L2), and waiting
                // for them here rather than at the end of the last chunk hides them behind phases 0 and 1.
                if (rc != d.r_begin) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                // Four strides of entries at a time: their key and count loads are in flight together (a big partition
                // of a hot bucket streams thousands of entries per chunk; one dependent load per stride was most
                // of this kernel's time at k31/b11).
                for (u32 e0 = 0; e0 < n_exist; e0 += 4 * 64) {
                    u64 klo[4], khi[4];
                    uint8_t cnt[4];
#pragma unroll
                    for (u32 q = 0; q < 4; q++) {
                        const u32 e = e0 + q * 64 + lane;
                        const unsigned long long at = off + (e < n_exist ? e : 0);
                        const u128x kq = load_key<KW>(ix, at);
                        klo[q] = kq.lo;
                        khi[q] = kq.hi;
                        cnt[q] = ix.counts[at];
                    }
#pragma unroll
                    for (u32 q = 0; q < 4; q++) {
                        const u32 e = e0 + q * 64 + lane;
                        if (e >= n_exist) continue;
                        u32 h = hash_key32(mk128(klo[q], khi[q])) & (tsize - 1);
                        for (;;) {
                            const u32 v = s_tab[h];
                            if (v == EMPTY_SLOT) break;
                            const u32 i = v & WI_IDX_MASK;
                            if (s_key[2 * i] == klo[q] && s_key[2 * i + 1] == khi[q]) {
                                ix.counts[off + e] = (uint8_t)count8<SAT>(cnt[q] + ((v & ~MATCHED_BIT) >> WI_CNT_SHIFT));
                                s_tab[h] = v | MATCHED_BIT;
                                break;
                            }
                            h = (h + 1) & (tsize - 1);
                        }
                    }
                }
                wave_sync();

                PHASE(5)
                // ---- 3. append the unmatched ones.  Generic body: the table is swept, the new entries' table words are
                // compacted in LDS and written out by full waves.  Compile-time geometry: every lane still holds its
                // instances' keys and slots and knows which of them created their slot, so the new entries are ranked with
                // one ballot per instance slot and written straight from registers -- no sweep of the table (8 rounds for
                // 512 slots), no list, no keys read back from LDS: 160 -> ~75 vector instructions per partition.
                u32 n_new = 0;
                u32 new_mask = 0, new_rank[NI], new_word[NI];
                if (NW) {
#pragma unroll
                    for (u32 it = 0; it < NI; it++) {
                        new_rank[it] = 0;
                        new_word[it] = 0;
                        if (it * 64 < ninst) {  // wave-uniform
                            const bool made = (li.won >> it) & 1;
                            if (made) new_word[it] = s_tab[li.hh[it]];
                            const bool is_new = made && !(new_word[it] & MATCHED_BIT);
                            const unsigned long long bal = __ballot(is_new);
                            new_rank[it] = n_new + (u32)__popcll(bal & lanes_below(lane));
                            if (is_new) new_mask |= 1u << it;
                            n_new += (u32)__popcll(bal);
                        }
                    }
                } else {
#pragma unroll
                    for (u32 w = 0; w < TS; w++) {
                        if (w * 64 < tsize) {
                            const u32 v = s_tab[w * 64 + lane];
                            const bool is_new = v != EMPTY_SLOT && !(v & MATCHED_BIT);
                            const unsigned long long bal = __ballot(is_new);
                            if (is_new) s_list[n_new + (u32)__popcll(bal & lanes_below(lane))] = v;
                            n_new += (u32)__popcll(bal);
                        }
                    }
                }
                wave_sync();
#ifndef INSERT_NO_EARLY_WAIT
                // The prefetched records are waited for HERE, before this chunk's stores are issued: vmcnt retires in issue
                // order, so a wait placed behind the stores (the next partition's first use) would sit out the stores' round
                // trip as well.  They were requested a partition's worth of work ago.
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
#endif

                PHASE(6)
                CNT(6, (n_new + 63) / 64)
                CNT(7, n_new)
                inst_left -= raw_inst;
                if (n_exist + n_new > cap) {
                    // move to a fresh slice, sized so that this partition moves at most once per batch
                    const unsigned long long want = grow_cap(n_exist + n_new + inst_left);
                    unsigned long long noff;
                    if (want > ARENA_CHUNK / 8) {
                        // a large slice goes straight to the global cursor: the private chunk never strands more
                        // than a small request (< ARENA_CHUNK/8) at a refill, which the host's reserve covers
                        unsigned long long got = 0;
                        if (lane == 0) got = atomicAdd(ix.cursor, want);
                        noff = __shfl(got, 0, 64);
                    } else {
                        if (acur + want > aend) {  // private chunk exhausted: abandon its tail, take a new one
                            garbage += aend - acur;
                            unsigned long long got = 0;
                            if (lane == 0) got = atomicAdd(ix.cursor, (unsigned long long)ARENA_CHUNK);
                            acur = __shfl(got, 0, 64);
                            aend = acur + ARENA_CHUNK;
                        }
                        noff = acur;
                        acur += want;
                    }
                    if (noff + want > ix.arena_cap || ninst > MAXI) {  // must not happen (host reserves the bound): drop, flag
                        if (lane == 0) atomicOr(ix.err, ninst > MAXI ? 4u : 2u);
                        break;
                    }
                    garbage += cap;
                    cap = (u32)want;
                    for (u32 e = lane; e < n_exist; e += 64) {
                        move_key<KW>(ix, noff + e, off + e);
                        ix.counts[noff + e] = ix.counts[off + e];
                    }
                    off = noff;
                }
                PHASE(7)
                if (NW) {
#pragma unroll
                    for (u32 it = 0; it < NI; it++) {
                        if ((new_mask >> it) & 1) {
                            const unsigned long long at = off + n_exist + new_rank[it];
                            store_key<KW>(ix, at, li.klo[it], li.khi[it]);
                            ix.counts[at] = (uint8_t)count8<SAT>(new_word[it] >> WI_CNT_SHIFT);  // (a new entry's word has no MATCHED_BIT)
                            const u32 bl = P.shift ? ((u32)shr128(mk128(li.klo[it], li.khi[it]), kbits).lo & ((1u << P.shift) - 1)) : 0;
                            const u32 bb = P.shift > 6 ? (bl >> (P.shift - 6)) : bl;  // 64 bins at most
                            if (bb < 32) bm0 |= 1u << bb; else bm1 |= 1u << (bb - 32);
                        }
                    }
                } else {
                    for (u32 q = lane; q < n_new; q += 64) {
                        const u32 v = s_list[q];
                        const u32 i = v & WI_IDX_MASK;
                        const u64 klo2 = s_key[2 * i], khi2 = s_key[2 * i + 1];
                        const unsigned long long at = off + n_exist + q;
                        store_key<KW>(ix, at, klo2, khi2);
                        ix.counts[at] = (uint8_t)count8<SAT>(v >> WI_CNT_SHIFT);
                        // bucket id inside the partition: the key's top `shift` bits (<= 6 of them used here)
                        const u32 bl = P.shift ? ((u32)shr128(mk128(klo2, khi2), kbits).lo & ((1u << P.shift) - 1)) : 0;
                        const u32 bb = P.shift > 6 ? (bl >> (P.shift - 6)) : bl;  // 64 bins at most
                        if (bb < 32) bm0 |= 1u << bb; else bm1 |= 1u << (bb - 32);
                    }
                }
                n_exist += n_new;
                rc += nrec;
                PHASE(8)

            }
            if (P.shift <= 6) {  // OR the lanes' bucket bits together on the DPP network (an LDS atomicOr on one word is turned
                                 // by the compiler into a scalar loop over the active lanes: 64 rounds per partition)
                bm0 = wave_or_all(bm0);
                if (P.shift == 6) bm1 = wave_or_all(bm1);
            }
            if (lane == 0) ix.dir[part] = DirEnt{off, n_exist, cap};
            // bucket occupancy bits: exact when a partition holds <= 64 buckets (shift <= 6);
            // partitions of more buckets are handled by k_bucket_bits below
            if (P.shift <= 6 && lane < 2) {
                const u32 mask = lane == 0 ? bm0 : bm1;
                const u32 nb = 1u << P.shift;  // buckets per partition
                const u64 first = ((u64)part << P.shift) >> P.ext_bits;  // ext_bits > 0 => shift == 0: the one bucket this partition is a slice of
                // With few buckets (small b) every partition of a bucket would hit the same word, and same-address atomics
                // serialise device-wide: there a bit that is already set is not set again (bits_check).  With many buckets
                // the words are all different, and the read before the atomic would be a dependent load behind this
                // partition's stores: the wave would sit out their whole round trip (it was a third of k_insert's time).
                if (mask) {
                    if (nb >= 32) {
                        if (lane * 32 < nb && (!ix.bits_check || (ix.bucket_bits[(first >> 5) + lane] & mask) != mask)) atomicOr(&ix.bucket_bits[(first >> 5) + lane], mask);
                    } else if (lane == 0) {
                        const u32 bits = mask << (first & 31);
                        if (!ix.bits_check || (ix.bucket_bits[first >> 5] & bits) != bits) atomicOr(&ix.bucket_bits[first >> 5], bits);
                    }
                }
            }
            } while (0);
            NEXT_PARTITION
#undef NEXT_PARTITION
            PHASE(9)
        }
    }
    PHASE_FLUSH
    if (lane == 0) {
        ix.slot_cur[blockIdx.x] = acur;
        ix.slot_end[blockIdx.x] = aend;
        if (garbage) atomicAdd(&ix.stats[3], garbage);
    }
}


#ifndef WI_WAVES_PER_EU_FAST
// Five waves per SIMD (<= 96 registers, 20 waves per CU: what the LDS holds at 7.7 KB a wave).  The body needs 115 since the
// next partition's records share the current ones' registers (127 before: 18 spilled at 96 and five waves gained nothing);
// at 96 it spills 10 to scratch and the fifth wave is worth it: 29.8 -> 26.3 ms per 50 M reads (5120 resident waves).
#define WI_WAVES_PER_EU_FAST 5
#endif
template <u32 NW, u32 KB, u32 SHIFT, bool SAT = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WI_WAVES_PER_EU_FAST, 8))) k_insert_fast(BriskParams P, RecSrc src, const PartDesc* __restrict__ desc,
                                                                                                        u32 n_touched, IndexDev ix, u32* __restrict__ work_counter) {
    static_assert(NW > 0, "compile-time record geometry");
    insert_body<WI_MAX_INST, NW, KB, SHIFT, SAT>(P, src, desc, n_touched, ix, work_counter);
}
// the same over a device-side list of descriptor indices (what k_insert_first left over; n_touched: the list's capacity)
template <u32 NW, u32 KB, u32 SHIFT, bool SAT = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WI_WAVES_PER_EU_FAST, 8))) k_insert_fast_listed(BriskParams P, RecSrc src, const PartDesc* __restrict__ desc,
                                                                                                               u32 n_touched, IndexDev ix, u32* __restrict__ work_counter,
                                                                                                               const u32* __restrict__ list, const u32* __restrict__ n_list) {
    insert_body<WI_MAX_INST, NW, KB, SHIFT, SAT, true>(P, src, desc, n_touched, ix, work_counter, list, n_list);
}
template <u32 NW, u32 KB, u32 SHIFT, bool SAT = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WI_WAVES_PER_EU, 8))) k_insert(BriskParams P, RecSrc src, const PartDesc* __restrict__ desc,
                                               u32 n_touched, IndexDev ix, u32* __restrict__ work_counter) {
    insert_body<WI_MAX_INST, NW, KB, SHIFT, SAT>(P, src, desc, n_touched, ix, work_counter);
}
template <u32 NW, u32 KB, u32 SHIFT, bool SAT = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 8))) k_insert_big(BriskParams P, RecSrc src, const PartDesc* __restrict__ desc,
                                                                                         u32 n_touched, IndexDev ix, u32* __restrict__ work_counter) {
    insert_body<2 * WI_MAX_INST, NW, KB, SHIFT, SAT>(P, src, desc, n_touched, ix, work_counter);
}

// ---- k_insert_first: the first fill of empty partitions (DESIGN.md section 4 finding 16).  The first batch into a fresh index
// (every one-shot job, and the flagship job at every step) finds every partition empty and -- folded -- nearly every one within
// one small chunk, yet insert_body keeps registers and LDS for four instance slots per lane, a stream over the existing entries,
// MATCHED_BIT, the move to a larger slice and the chunk loop.  This body has none of them: NI_LEAN instance slots per lane,
// one chunk, every slot a lane won is a new entry.  It is built from insert_body's pieces and yields, for a partition it takes,
// exactly what insert_body yields: the same entries in the same order in a slice of the same capacity.  A partition it must not
// take -- not empty, more than 64 records, more than 64 * NI_LEAN instances after the fold -- is left over: before anything
// global is written for it, its descriptor index goes to a list that k_insert_fast then walks (one atomic per batch of WI_BATCH
// partitions: the batch's left-over partitions are a 64-bit mask in scalar registers).
#ifndef NI_LEAN
#define NI_LEAN 3   // k_insert_first's default slot count: profiles/r13_insert_ninst.txt, r17_insert_ninst.txt (-DNI_LEAN=2: the two-slot kernel, for A/B)
#endif
#ifndef WI_WAVES_PER_EU_FIRST
#define WI_WAVES_PER_EU_FIRST 6
#endif
#ifndef WI_WAVES_PER_EU_FIRST_MAX
#define WI_WAVES_PER_EU_FIRST_MAX 6
#endif
template <u32 NIL, u32 NW>
struct LeanLds {
    // TABLE: the probe masks with tsize - 1, so a power of two.  512 slots are four per instance up to 128 instances and 2.7 at
    // 192 (insert_body: two at 256); 4 * MAXI = 768 at three slots would let tsize double past it to 1024, 640 B beyond s_mem.
    static constexpr u32 MAXI = 64 * NIL, TABLE = 512;
    static_assert((TABLE & (TABLE - 1)) == 0 && TABLE >= 2 * MAXI && TABLE <= 4 * MAXI, "probe table: a power of two, at most half full");
    static constexpr u32 REC_BYTES = (WI_MAX_REC * RecGeom<NW>::RS + 4) * 4;   // shifted record words, + 4: the last record's window
    static constexpr u32 OFF_REC = 16 * MAXI;                                  // keys first (s_idiff over them)
    static constexpr u32 REGION = REC_BYTES > 4 * TABLE ? REC_BYTES : 4 * TABLE;  // the probe table lies over the records
    static constexpr u32 OFF_IREC = OFF_REC + REGION, OFF_IMULT = OFF_IREC + MAXI, BYTES = OFF_IMULT + MAXI;
};
__device__ __forceinline__ unsigned long long first_lane64(unsigned long long v) {
    return ((unsigned long long)(u32)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)v);
}
// ---- Two small partitions in one wave (section 4 finding 22).  The flagship job's partitions hold 12 records on 64 lanes, and most
// of what the body issues per partition does not depend on how many lanes hold something.  Where the next two descriptors A and B of
// the wave's batch are both first-fill candidates (empty, no slice, not huge) with n_rec(A) + n_rec(B) <= 64, B's records are loaded
// behind A's -- lanes [nA, nA + nB) -- and the two run one fold (ck carries a partition bit, so a record meets only heads of its own
// partition), one instance map, one table-free expansion and one store tail with two slices, two directory entries and two
// bucket_bits words.  The pair goes on only where the joint grouped fold stands, both partitions are clean and their instances
// together are at most MAXI; otherwise A goes alone -- from the joint fold's results for its lanes, which are what its own fold
// yields, groups do not interact; from the top where the joint fold did not stand -- and B heads the next candidate pair.
// Entries, their order and each cap are what the single route yields; only the slices' places in the arena may differ.
#ifndef INSERT_PAIR
#define INSERT_PAIR 1   // -DINSERT_PAIR=0: the single-partition body alone, for A/B
#endif
#define PAIR_B_BIT 18u  // ck's partition bit, above [routing id low bits (SHIFT <= 4) | core (14)]
// a pair's records: lane r < nA loads record r of partition A, lane nA + r (r < nB) record r of partition B (nB == 0: load_part_recs)
__device__ __forceinline__ RecRegs load_pair_recs(const BriskParams& P, const RecSrc& src, u32 part_a, u32 begin_a, u32 nA, u32 part_b, u32 begin_b, u32 nB, u32 lane) {
    RecRegs r{0, 0, 0, 0, 0};
    // (everything per partition is wave-uniform, in scalar registers: record 0 of the bin -- classic: of the partition -- and the
    // place record 0 would have in the overflow area; a lane picks one of the four and adds its record's index)
    const u32 in_bin = src.bin_cap ? src.bin_cap : ~0u;
    const u64 bytes = (u64)P.stride * 8, rec0 = (u64)(uintptr_t)src.rec, ovf0 = (u64)(uintptr_t)src.ovf;
    const u64 bin_a = rec0 + (src.bin_cap ? (u64)part_a * src.bin_cap : (u64)begin_a) * bytes, ovf_a = ovf0 + ((u64)begin_a - src.bin_cap) * bytes;
    const u64 bin_b = rec0 + (src.bin_cap ? (u64)part_b * src.bin_cap : (u64)begin_b) * bytes, ovf_b = ovf0 + ((u64)begin_b - src.bin_cap) * bytes;
    if (lane < nA + nB) {
        const bool is_b = lane >= nA;
        const u32 i = is_b ? lane - nA : lane;
        const u64 base = i < in_bin ? (is_b ? bin_b : bin_a) : (is_b ? ovf_b : ovf_a);
        const u64* c = (const u64*)(uintptr_t)(base + i * bytes);
        r.w0 = c[0];
        r.w1 = c[1];
        if (P.stride > 2) r.w2 = c[2];
        if (P.stride > 3) r.w3 = c[3];
        if (P.stride > 4) r.w4 = c[4];
    }
    return r;
}
template <u32 NIL, u32 NW, u32 KB, u32 SHIFT, bool SAT>
__device__ __forceinline__ void insert_first_body(const BriskParams& P, const RecSrc& src, const PartDesc* __restrict__ desc, u32 n_touched, const IndexDev& ix,
                                                  u32* __restrict__ work_counter, u32* __restrict__ left_list, u32* __restrict__ n_left, u32* __restrict__ n_clean,
                                                  u32* __restrict__ n_pair) {
    using L = LeanLds<NIL, NW>;
    constexpr u32 MAXI = L::MAXI, TABLE = L::TABLE, RS = RecGeom<NW>::RS, INFO = RecGeom<NW>::INFO, KBITS = 2 * KB + 6;
    constexpr u32 KW = KBITS + SHIFT <= 64 ? 1u : 2u;
    // The table-free path (finding 19): where the fold proves that a partition's instances are all distinct (fold_records, DETECT),
    // instance i is entry i with the multiplicity s_imult holds -- what the probe table yields for it, every instance winning its
    // slot -- and hashing, the key copies in LDS, the table, its rounds and the ranking are left out.  The core mask is the
    // flagship geometry's: k63 m21 b14 (any other m with k - b = 49 takes the table path); n_clean == nullptr switches the path off.
    constexpr u32 CORE_K = 63, CORE_M = 21, CORE_B = 14, CW = CORE_K - CORE_M;
    static_assert(KB == CORE_K - CORE_B, "fold_core: the core of k63 m21 b14");
    static_assert(NIL == 2 || NIL == 3, "instance slots per lane");
    static_assert(NW >= 3 && SHIFT < 5, "the folding k63 geometries: at most 16 buckets per partition");
    static_assert(L::BYTES <= 13 * 512, "LDS per wave: 24 waves must fit a CU's 160 KiB");
    static_assert(4 * MAXI <= 16 * MAXI, "the multiplicity steps lie over the keys");
    static_assert(MAXI + (MAXI >> 2) + 8 <= ARENA_CHUNK / 8, "grow_cap(MAXI) is a small request: the host's arena reserve covers the tail a refill strands");
    __shared__ __attribute__((aligned(16))) unsigned char s_mem[L::BYTES];
    u64* s_key = (u64*)s_mem;
    u32* s_idiff = (u32*)s_mem;
    u32* s_rw = (u32*)(s_mem + L::OFF_REC);
    u32* s_tab = (u32*)(s_mem + L::OFF_REC);
    uint8_t* s_irec = s_mem + L::OFF_IREC;
    uint8_t* s_imult = s_mem + L::OFF_IMULT;

    const u32 lane = threadIdx.x;
    PHASE_DECL
    // the wave's private arena chunk: wave-uniform, in scalar registers
    unsigned long long acur = first_lane64(ix.slot_cur[blockIdx.x]), aend = first_lane64(ix.slot_end[blockIdx.x]), garbage = 0;
    const u32 frame_end = P.suff_reduc + P.w + 1;
    // the idx' from which on a window covers the core; beyond every idx' (no record is sure, no partition table-free) where the path is off
    const u32 core_from = (n_clean != nullptr && P.w == CW) ? P.suff_reduc : 0x100u;
    // pairs only where the table-free path is on: a pair has no table path
    const bool pair_on = INSERT_PAIR && n_pair != nullptr && core_from != 0x100u;
    // Requests the records of head `a` (descriptor index ta) and, where the pair rule holds for desc[ta] and desc[ta + 1], of its
    // neighbour behind them; returns the neighbour's record count, 0 where `a` goes alone.  B must lie inside the batch.
    auto request = [&](const PartDesc& a, u32 ta, u32 t_end, RecRegs& rr) -> u32 {
        u32 nB = 0, part_b = 0, begin_b = 0;
        if (pair_on && ta + 1 < t_end && !(a.n_exist | a.cap) && a.n_rec - 1u < (u32)WI_MAX_REC - 1u && !(ix.huge_at && a.n_inst > ix.huge_at)) {
            const PartDesc b = desc[ta + 1];
            if (!(b.n_exist | b.cap) && b.n_rec != 0 && a.n_rec + b.n_rec <= (u32)WI_MAX_REC && !(ix.huge_at && b.n_inst > ix.huge_at)) {
                nB = b.n_rec;
                part_b = b.part;
                begin_b = b.r_begin;
            }
        }
        // (one load for both cases: alone, no lane lies in B's range)
        rr = load_pair_recs(P, src, a.part, a.r_begin, min(a.n_rec, (u32)WI_MAX_REC), part_b, begin_b, nB, lane);
        return nB;
    };

    for (;;) {
        u32 t0 = 0;
        if (lane == 0) t0 = atomicAdd(work_counter, WI_BATCH);
        t0 = (u32)__builtin_amdgcn_readfirstlane((int)t0);
        if (t0 >= n_touched) break;
        const u32 t_end = min(t0 + WI_BATCH, n_touched);
        unsigned long long left_mask = 0;  // partitions t0 + i of this batch that are left to k_insert_fast (wave-uniform)
        unsigned long long clean_mask = 0;  // those that took the table-free path (counted for the trace)
        u32 pairs = 0;                      // partitions of this batch taken in pairs
        PartDesc d = desc[t0];
        RecRegs rr;
        u32 nB = INSERT_PAIR ? request(d, t0, t_end, rr) : 0u;  // records of desc[t + 1] behind d's in rr (0: d alone)
        if (!INSERT_PAIR) rr = load_part_recs(P, src, d.part, d.r_begin, d.r_begin, min(d.n_rec, (u32)WI_MAX_REC), lane);

        for (u32 t = t0, step = 1; t < t_end; t += step) {
            u32 tn = t + 1;
            step = 1;
            PartDesc dn{};
            if (tn < t_end) dn = desc[tn];  // (of a pair: B's)
            // (the records of the next partition are requested at the end of this one, and must have landed on every path: insert_body)
            asm volatile("" ::"v"(rr.w0), "v"(rr.w1), "v"(rr.w2), "v"(rr.w3), "v"(rr.w4));
            do {
                if (ix.huge_at && d.n_inst > ix.huge_at) break;  // k_insert_huge takes this one
                CNT(0, 1)
                if (d.n_exist | d.cap | (u32)(d.n_rec > WI_MAX_REC)) {
                    left_mask |= 1ull << (t - t0);
                    break;
                }
                PHASE(0)
                const u32 part = d.part, nA = d.n_rec;
                u32 nrec = nA + nB;  // (the pair rule: at most WI_MAX_REC)
                const u64 my_hdr = NW == 3 ? rr.w3 : rr.w4;
                const u32 raw_n = lane < nrec ? hdr_n(my_hdr) : 0;
                const u32 my_mult = (my_hdr & HDR_HAS_MULT) ? (u32)(my_hdr >> 48) & 0xffu : 1u;
                const u32 info_hi = (raw_n << 10) | (hdr_idx0(my_hdr) << 18) | ((hdr_bucket(my_hdr) & ((1u << SHIFT) - 1)) << 26);
                const FoldFrame ff = fold_frame<NW, KB>(rr, my_hdr, raw_n, lane < nrec, frame_end, lane);
                wave_sync();  // the previous partition has read its table
                if (lane < nrec) store_rec_words<NW>(s_rw + lane * RS, rr, 0);
                u32 lead = lane, lead_off = 0, dbg_trips = 0;
                // (a record that takes no part in the fold, or reaches below suff_reduc: its windows may miss the core)
                const bool unsure_any = ff.s == 0 || hdr_idx0(my_hdr) < core_from;
                bool clean = false;
                // (of a pair: B's lanes carry the partition bit, so equal ck stays equal routing id; alone, no lane below nrec has it)
                const u32 ck = ((hdr_bucket(my_hdr) & ((1u << SHIFT) - 1)) << (2 * (KB - CW))) | fold_core<KB, CW>(ff.u) |
                               (INSERT_PAIR && lane >= nA ? 1u << PAIR_B_BIT : 0u);
                static_assert(SHIFT + 2 * (KB - CW) <= PAIR_B_BIT, "ck: the partition bit lies above the routing id's low bits and the core");
                bool dup = false;
                unsigned long long dirty_lanes = 0;
                // (the slot words lie over s_key / s_idiff, which nothing holds before the instance map below)
                for (;;) {  // wave-uniform; a second turn only where the joint fold of a pair does not stand: A alone, from the top
                    const bool unsure = lane < nrec && unsure_any;
                    if (FOLD_GROUPED && fold_records_grouped<NW>(ff, nrec, lane, (u32*)s_mem, &lead, &lead_off, &dup, &dbg_trips, ck, unsure, &clean, &dirty_lanes)) break;
                    if (INSERT_PAIR && nB) {
                        nB = 0;
                        nrec = nA;
                        continue;
                    }
                    dup = fold_records<NW, true>(ff, nrec, lane, &lead, &lead_off, &dbg_trips, ck, unsure, &clean);
                    break;
                }
#ifdef INSERT_ATTR_NOTABLE  // attribution build: every partition taken goes down the table-free path.  Wrong results, timing only
                clean = true;
#endif
                u32 my_n = (lane < nrec && !dup) ? raw_n : 0;
                const u32 x = wave_incl_scan(my_n, lane);
                u32 ninst = (u32)__builtin_amdgcn_readlane((int)x, 63);
                u32 ninstA = ninst;  // (of a pair: A's instances are [0, ninstA) of the joint list, B's the rest)
                if (INSERT_PAIR && nB) {  // wave-uniform: pair or not, decided after the fold
                    ninstA = (u32)__builtin_amdgcn_readlane((int)x, (int)(nA - 1));
                    const bool clean_a = (dirty_lanes & ((1ull << nA) - 1)) == 0;
                    if (clean && ninst <= MAXI) {  // (clean: no lane of either is dirty)
                        step = 2;
                        pairs += 2;
                    } else {  // A alone, from the joint fold's results for its lanes; B heads the next candidate pair
                        nB = 0;
                        nrec = nA;
                        clean = clean_a;
                        if (lane >= nA) my_n = 0;
                        ninst = ninstA;
                    }
                }
                if (ninst > MAXI) {  // (nothing but LDS has been written)
                    left_mask |= 1ull << (t - t0);
                    break;
                }
                PHASE(1)
                CNT(1, 1)
                const u32 m_first = (u32)__shfl(x - my_n, lead, 64) + lead_off;
                u32 tsize = 128;
                while (tsize < 4 * ninst && tsize < TABLE) tsize <<= 1;
                {
                    // instance -> record and every instance's multiplicity, as in insert_body; a lane owns NIL consecutive instances
                    if (NIL == 2) ((uint16_t*)s_irec)[lane] = 0;
                    else {
#pragma unroll
                        for (u32 q = 0; q < NIL; q++) s_irec[q * 64 + lane] = 0;
                    }
#pragma unroll
                    for (u32 q = 0; q < NIL; q++) s_idiff[lane * NIL + q] = 0;
                    wave_sync();
                    if (my_n) s_irec[x - my_n] = (uint8_t)(lane + 1);
                    if (lane < nrec) {
                        atomicAdd(&s_idiff[m_first], my_mult);
                        // (of a pair the map runs over the concatenated list unchanged: a record of A that ends on A's last instance
                        // steps down at ninstA < ninst, B's first instance, so the running sum is back at zero where B begins)
                        if (m_first + raw_n < ninst) atomicAdd(&s_idiff[m_first + raw_n], 0u - my_mult);
                    }
                    wave_sync();
                    u32 mk[NIL], mv[NIL], run = 0, tot = 0;
                    if (NIL == 2) {
                        const u32 w = ((const uint16_t*)s_irec)[lane];
                        mk[0] = w & 0xff;
                        mk[1] = w >> 8;
                    } else {
#pragma unroll
                        for (u32 q = 0; q < NIL; q++) mk[q] = s_irec[lane * NIL + q];
                    }
#pragma unroll
                    for (u32 q = 0; q < NIL; q++) {
                        run = op_max_u32(run, mk[q]);
                        tot += s_idiff[lane * NIL + q];
                        mv[q] = tot;
                    }
                    const u32 before = wave_incl_scan(tot, lane) - tot;
                    u32 carry = wave_prev_lane(wave_incl_max_scan(run));  // the last mark before this lane's instances
#pragma unroll
                    for (u32 q = 0; q < NIL; q++) {
                        carry = op_max_u32(carry, mk[q]);
                        mk[q] = (carry - 1) & 0xff;  // marks are lane + 1; instances past the last record (none are read) may hold 0 - 1
                        mv[q] = count8<SAT>(mv[q] + before) & 0xff;
                    }
                    if (NIL == 2) {
                        ((uint16_t*)s_irec)[lane] = (uint16_t)(mk[0] | (mk[1] << 8));
                        ((uint16_t*)s_imult)[lane] = (uint16_t)(mv[0] | (mv[1] << 8));
                    } else {
#pragma unroll
                        for (u32 q = 0; q < NIL; q++) {
                            s_irec[lane * NIL + q] = (uint8_t)mk[q];
                            s_imult[lane * NIL + q] = (uint8_t)mv[q];
                        }
                    }
                    // the records' info words: [first instance | n | idx0' | routing id low bits]
                    if (lane < nrec) s_rw[lane * RS + INFO] = (x - my_n) | info_hi;
                }
                wave_sync();
                PHASE(2)
                CNT(3, (ninst + 63) / 64)
                CNT(4, ninst)
                CNT(5, nrec)
                CNT(11, dbg_trips)
                u32 dbg_r = 0;
                LaneInst<NIL> li;
                li.won = 0;
                u32 n_new = 0, new_rank[NIL], new_word[NIL];
                if (clean) {  // wave-uniform: the table-free path.  Instance i is entry i, its count what s_imult holds
                    clean_mask |= (INSERT_PAIR && nB ? 3ull : 1ull) << (t - t0);
                    // (the lane as this path sees it, opaque: what is derived from it here is computed here, not kept in registers
                    // from before the partition loop, where the table path's own addresses already fill the 80)
                    u32 ln = lane;
                    asm volatile("" : "+v"(ln));
                    if (ninst <= 64) expand_words_distinct<1, NW, KB, SHIFT, NIL>(ln, ninst, s_rw, s_irec, li);
                    else if (NIL == 2 || ninst <= 128) expand_words_distinct<2, NW, KB, SHIFT, NIL>(ln, ninst, s_rw, s_irec, li);
                    else expand_words_distinct<NIL, NW, KB, SHIFT, NIL>(ln, ninst, s_rw, s_irec, li);
                    n_new = ninst;
#pragma unroll
                    for (u32 it = 0; it < NIL; it++) {
                        const u32 i = it * 64 + ln;
                        new_rank[it] = i;
                        new_word[it] = (u32)s_imult[i < ninst ? i : 0] << WI_CNT_SHIFT;
                    }
                    PHASE(3)
                } else {
                    if (ninst <= 64) expand_and_dedupe_words<1, NW, KB, SHIFT, NIL, true, SAT>(lane, ninst, tsize, s_rw, s_irec, s_imult, nullptr, s_key, s_tab, &dbg_r, li);
                    else if (NIL == 2 || ninst <= 128) expand_and_dedupe_words<2, NW, KB, SHIFT, NIL, true, SAT>(lane, ninst, tsize, s_rw, s_irec, s_imult, nullptr, s_key, s_tab, &dbg_r, li);
                    else expand_and_dedupe_words<NIL, NW, KB, SHIFT, NIL, true, SAT>(lane, ninst, tsize, s_rw, s_irec, s_imult, nullptr, s_key, s_tab, &dbg_r, li);
                    wave_sync();
                    CNT(8, dbg_r)
                    PHASE(3)
                    // ---- the new entries: every slot a lane created, ranked with one ballot per instance slot
#pragma unroll
                    for (u32 it = 0; it < NIL; it++) {
                        new_rank[it] = 0;
                        new_word[it] = 0;
                        if (it * 64 < ninst) {  // wave-uniform
                            const bool made = (li.won >> it) & 1;
                            if (made) new_word[it] = s_tab[li.hh[it]];
                            const unsigned long long bal = __ballot(made);
                            new_rank[it] = n_new + (u32)__popcll(bal & lanes_below(lane));
                            n_new += (u32)__popcll(bal);
                        }
                    }
                }
                wave_sync();
#ifndef INSERT_NO_EARLY_WAIT
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the prefetched records, before this partition's stores (insert_body)
#endif
                PHASE(6)
                CNT(7, n_new)
                // the slice insert_body takes for a fresh partition of one chunk, from the private chunk (of a pair: A's, then B's,
                // a refill may fall between the two); n: the partition's new entries, 0 where the slice could not be had
                auto take_slice = [&](u32& n, unsigned long long& off, u32& cap) {
                    cap = 0;
                    if (n) {
                        const unsigned long long want = grow_cap(n);  // <= grow_cap(MAXI) = 248 at three slots: far below ARENA_CHUNK / 8 (asserted above)
                        if (acur + want > aend) {
                            garbage += aend - acur;
                            unsigned long long got = 0;
                            if (lane == 0) got = atomicAdd(ix.cursor, (unsigned long long)ARENA_CHUNK);
                            acur = first_lane64(got);
                            aend = acur + ARENA_CHUNK;
                        }
                        if (acur + want > ix.arena_cap) {  // must not happen (the host reserves the bound): drop, flag
                            if (lane == 0) atomicOr(ix.err, 2u);
                            n = 0;
                        } else {
                            off = acur;
                            acur += want;
                            cap = (u32)want;
                        }
                    }
                };
                if (INSERT_PAIR && nB) {  // wave-uniform: the pair's tail, a block of its own (the single tail below is the parent's)
                    // instance i is entry i of A's slice, or entry i - ninstA of B's; B's bucket bits go to the high half of the word
                    unsigned long long off = d.off, off_b = dn.off;
                    u32 cap = 0, cap_b = 0, n_new_b = n_new - ninstA;
                    n_new = ninstA;
                    take_slice(n_new, off, cap);
                    take_slice(n_new_b, off_b, cap_b);
                    u32 ln = lane, bm0 = 0;
                    asm volatile("" : "+v"(ln));
#pragma unroll
                    for (u32 it = 0; it < NIL; it++) {
                        const u32 i = it * 64 + ln;
                        const bool in_b = i >= ninstA;
                        if (i < ninst && (in_b ? n_new_b : n_new)) {
                            const unsigned long long at = (in_b ? off_b - ninstA : off) + i;
                            store_key<KW>(ix, at, li.klo[it], li.khi[it]);
                            ix.counts[at] = (uint8_t)count8<SAT>(new_word[it] >> WI_CNT_SHIFT);
                            const u32 bl = (u32)shr128(mk128(li.klo[it], li.khi[it]), KBITS).lo & ((1u << SHIFT) - 1);
                            bm0 |= 1u << (bl + (in_b ? 16u : 0u));  // (this form: the others tried cost two registers beyond the 80)
                        }
                    }
                    bm0 = wave_or_all(bm0);
                    if (ln == 0) {
                        ix.dir[part] = DirEnt{off, n_new, cap};
                        ix.dir[dn.part] = DirEnt{off_b, n_new_b, cap_b};
                        const u64 first = ((u64)part << SHIFT) >> P.ext_bits, first_b = ((u64)dn.part << SHIFT) >> P.ext_bits;
                        const u32 bits = (bm0 & 0xffffu) << (first & 31), bits_b = (bm0 >> 16) << (first_b & 31);
                        if (bits && (!ix.bits_check || (ix.bucket_bits[first >> 5] & bits) != bits)) atomicOr(&ix.bucket_bits[first >> 5], bits);
                        if (bits_b && (!ix.bits_check || (ix.bucket_bits[first_b >> 5] & bits_b) != bits_b)) atomicOr(&ix.bucket_bits[first_b >> 5], bits_b);
                    }
                    break;
                }
                unsigned long long off = d.off;
                u32 cap = 0;
                take_slice(n_new, off, cap);
                PHASE(7)
                u32 bm0 = 0;
#pragma unroll
                for (u32 it = 0; it < NIL; it++) {
                    if (it * 64 < ninst && ((li.won >> it) & 1) && n_new) {
                        const unsigned long long at = off + new_rank[it];
                        store_key<KW>(ix, at, li.klo[it], li.khi[it]);
                        ix.counts[at] = (uint8_t)count8<SAT>(new_word[it] >> WI_CNT_SHIFT);
                        const u32 bl = SHIFT ? ((u32)shr128(mk128(li.klo[it], li.khi[it]), KBITS).lo & ((1u << SHIFT) - 1)) : 0;
                        bm0 |= 1u << bl;
                    }
                }
                PHASE(8)
                bm0 = wave_or_all(bm0);
                if (lane == 0) {
                    ix.dir[part] = DirEnt{off, n_new, cap};
                    // bucket occupancy bits (insert_body's epilogue, fewer than 32 buckets per partition)
                    const u64 first = ((u64)part << SHIFT) >> P.ext_bits;
                    const u32 bits = bm0 << (first & 31);
                    if (bits && (!ix.bits_check || (ix.bucket_bits[first >> 5] & bits) != bits)) atomicOr(&ix.bucket_bits[first >> 5], bits);
                }
            } while (0);
            if (INSERT_PAIR && step == 2) {  // wave-uniform: B went with A, the next head is the one behind it
                tn = t + 2;
                dn = PartDesc{};
                if (tn < t_end) dn = desc[tn];
            }
            d = dn;
            if (INSERT_PAIR) {
                nB = 0;
                if (tn < t_end) nB = request(d, tn, t_end, rr);
            } else if (tn < t_end) rr = load_part_recs(P, src, d.part, d.r_begin, d.r_begin, min(d.n_rec, (u32)WI_MAX_REC), lane);
            PHASE(9)
        }
        if (INSERT_PAIR && pairs && lane == 0) atomicAdd(n_pair, pairs);
        if (left_mask) {  // wave-uniform
            const u32 n = (u32)__popcll(left_mask);
            u32 at = 0;
            if (lane == 0) at = atomicAdd(n_left, n);
            at = (u32)__builtin_amdgcn_readfirstlane((int)at);
            // (once per batch: from an opaque copy of the lane, so that 1 << lane is not kept in two registers across every partition)
            u32 ln = lane;
            asm volatile("" : "+v"(ln));
            if ((left_mask >> ln) & 1) left_list[at + (u32)__popcll(left_mask & lanes_below(ln))] = t0 + ln;
        }
        if (clean_mask && n_clean && lane == 0) atomicAdd(n_clean, (u32)__popcll(clean_mask));
    }
    PHASE_FLUSH
    if (lane == 0) {
        ix.slot_cur[blockIdx.x] = acur;
        ix.slot_end[blockIdx.x] = aend;
        if (garbage) atomicAdd(&ix.stats[3], garbage);
    }
}
template <u32 NW, u32 KB, u32 SHIFT, bool SAT = false, u32 NIL = NI_LEAN>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WI_WAVES_PER_EU_FIRST, WI_WAVES_PER_EU_FIRST_MAX))) k_insert_first(BriskParams P, RecSrc src, const PartDesc* __restrict__ desc,
                                                                                                          u32 n_touched, IndexDev ix, u32* __restrict__ work_counter,
                                                                                                          u32* __restrict__ left_list, u32* __restrict__ n_left, u32* __restrict__ n_clean,
                                                                                                          u32* __restrict__ n_pair) {
    insert_first_body<NIL, NW, KB, SHIFT, SAT>(P, src, desc, n_touched, ix, work_counter, left_list, n_left, n_clean, n_pair);
}

// bucket occupancy for partitions wider than 64 buckets (small part_bits): one pass over all entries
__global__ void __launch_bounds__(256) k_bucket_bits(BriskParams P, IndexDev ix, u32 n_parts) {
    const u32 kbits = 2 * P.kb + 6;
    for (u32 part = blockIdx.x; part < n_parts; part += gridDim.x) {
        const u32 cnt = ix.dir[part].cnt;
        const unsigned long long off = ix.dir[part].off;
        for (u32 e = threadIdx.x; e < cnt; e += blockDim.x) {
            const u128x key = load_key(ix, off + e);
            const u32 bucket = (part << P.shift) | ((u32)shr128(key, kbits).lo & ((1u << P.shift) - 1));
            const u32 bit = 1u << (bucket & 31);
            if (!(ix.bucket_bits[bucket >> 5] & bit)) atomicOr(&ix.bucket_bits[bucket >> 5], bit);
        }
    }
}

// stats(): nb_kmers = sum dir_cnt, largest = max dir_cnt, nb_buckets = popcount(bucket_bits)
__global__ void __launch_bounds__(256) k_stats(const DirEnt* __restrict__ dir, u64 n_parts, const u32* __restrict__ bits, u64 n_words,
                                               unsigned long long* out /* [0] kmers [1] buckets [2] largest */) {
    __shared__ unsigned long long s_a[4], s_b[4], s_c[4];
    unsigned long long a = 0, b = 0, c = 0;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_parts; i += stride) {
        const u32 v = dir[i].cnt;
        a += v;
        c = v > c ? v : c;
    }
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += stride) b += __popc(bits[i]);
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o, 64);
        b += __shfl_down(b, o, 64);
        const unsigned long long c2 = __shfl_down(c, o, 64);
        c = c2 > c ? c2 : c;
    }
    if ((threadIdx.x & 63) == 0) {
        s_a[threadIdx.x >> 6] = a;
        s_b[threadIdx.x >> 6] = b;
        s_c[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&out[0], s_a[0] + s_a[1] + s_a[2] + s_a[3]);
        atomicAdd(&out[1], s_b[0] + s_b[1] + s_b[2] + s_b[3]);
        unsigned long long m = s_c[0];
        for (int i = 1; i < 4; i++) m = s_c[i] > m ? s_c[i] : m;
        atomicMax(&out[2], m);
    }
}


// ===========================================================================
// k_insert_huge: one WORKGROUP of 16 waves per partition, for the partitions one wave must not be left alone with: a hot
// minimizer (satellite repeats, poly-A) puts 10^5..10^6 distinct k-mers into ONE partition, which the wave-per-partition
// kernels work off in chunks of 256 / 512 instances, every chunk streaming the partition's entries through its table --
// entries x instances / 256 probes by 64 lanes while the rest of the device idles.  Here a chunk is 2048 instances in a
// table shared by 1024 lanes: 8 times fewer passes over the entries, each 16 times as wide.  Same semantics as insert_body
// (find-all then insert-missing, DenseMenuYo.hpp:248-310; counts wrap at 256, or with SAT stop at 255); run-time geometry; classic and binned record
// layouts.  Partitions are chosen by k_need (PartDesc::n_inst > IndexDev::huge_at); the wave kernels skip them.
#define HG_THREADS 1024u
#define HG_INST 2048u          // k-mer instances per chunk
#define HG_TAB 4096u           // table slots
#define HG_LIVE 0x80000000u    // s_cnt: the key owns a table slot (keys allocated by the losers of a CAS race stay dead)
#define HG_EXIST 0x40000000u   // s_cnt: an existing entry has this key
#define HG_MULT 0x3fffffffu
__device__ __forceinline__ const u64* huge_rec(const BriskParams& P, const RecSrc& src, const PartDesc& d, u32 i) {  // record i of the partition (RecSrc)
    if (!src.bin_cap) return src.rec + (u64)(d.r_begin + i) * P.stride;
    return i < src.bin_cap ? src.rec + ((u64)d.part * src.bin_cap + i) * P.stride : src.ovf + ((u64)d.r_begin + i - src.bin_cap) * P.stride;
}
// inclusive prefix sum over the block's 1024 lanes (wave scan + the waves' totals through LDS); *total: the block's sum
__device__ __forceinline__ u32 block_incl_scan(u32 v, u32* s_wsum, u32* total) {
    const u32 lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    u32 x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const u32 y = __shfl_up(x, o, 64);
        if ((int)lane >= o) x += y;
    }
    __syncthreads();  // s_wsum may still be read from the previous call
    if (lane == 63) s_wsum[wid] = x;
    __syncthreads();
    u32 before = 0, all = 0;
    for (u32 i = 0; i < HG_THREADS / 64; i++) {
        const u32 c = s_wsum[i];
        if (i < wid) before += c;
        all += c;
    }
    *total = all;
    return x + before;
}
template <bool SAT>
__global__ void __launch_bounds__(HG_THREADS) k_insert_huge(BriskParams P, RecSrc src, const PartDesc* __restrict__ desc, const u32* __restrict__ huge_list,
                                                            const u32* __restrict__ n_huge, IndexDev ix) {
    __shared__ u64 s_key[2 * HG_INST];
    __shared__ u32 s_tab[HG_TAB];
    __shared__ u32 s_cnt[HG_INST];
    __shared__ u32 s_pref[HG_THREADS + 1];
    __shared__ u32 s_wsum[HG_THREADS / 64];
    __shared__ u32 s_nkeys, s_bm[2], s_fail;
    __shared__ unsigned long long s_noff;
    const u32 tid = threadIdx.x;
    const u32 kbits = 2 * P.kb + 6;
    for (u32 hi = blockIdx.x; hi < *n_huge; hi += gridDim.x) {
        const PartDesc d = desc[huge_list[hi]];
        u32 n_exist = d.n_exist, cap = d.cap, inst_left = d.n_inst;
        unsigned long long off = d.off, garbage = 0;
        if (tid < 2) s_bm[tid] = 0;
        if (tid == 0) s_fail = 0;
        bool failed = false;
        for (u32 rc = 0; rc < d.n_rec && !failed;) {
            // ---- the chunk: the longest run of records (one per lane) with at most HG_INST instances
            const u32 avail = min(d.n_rec - rc, HG_THREADS);
            u32 my_n = 0;
            if (tid < avail) my_n = hdr_n(huge_rec(P, src, d, rc + tid)[P.nw]);
            u32 all;
            const u32 x = block_incl_scan(my_n, s_wsum, &all);
            s_pref[tid + 1] = x;
            if (tid == 0) {
                s_pref[0] = 0;
                s_nkeys = 0;
            }
            for (u32 i = tid; i < HG_TAB; i += HG_THREADS) s_tab[i] = EMPTY_SLOT;
            u32 nrec;
            (void)block_incl_scan(tid < avail && x <= HG_INST ? 1u : 0u, s_wsum, &nrec);  // a prefix: >= 1 (a record has <= 255 instances)
            __syncthreads();
            const u32 ninst = s_pref[nrec];
            // ---- expand and de-duplicate: every distinct key gets a slot in s_key / s_cnt and an entry in the table
            for (u32 i = tid; i < ninst; i += HG_THREADS) {
                u32 lo = 0, hi2 = nrec;  // the record r with s_pref[r] <= i < s_pref[r + 1]
                while (hi2 - lo > 1) {
                    const u32 mid = (lo + hi2) >> 1;
                    if (s_pref[mid] <= i) lo = mid; else hi2 = mid;
                }
                const u64* c = huge_rec(P, src, d, rc + lo);
                u64 w[5];
                for (u32 q = 0; q < 5; q++) w[q] = q <= P.nw ? c[q] : 0;
                const u64 hdr = w[P.nw];
                const u32 j = i - s_pref[lo];
                const u128x key = make_key(P, hdr_bucket(hdr), record_kmer(P, w, hdr_n(hdr), j), hdr_idx0(hdr) + j);
                const u32 mult = (hdr & HDR_HAS_MULT) ? (u32)(hdr >> 48) & 0xffu : 1u;
                u32 h = hash_key32(key) & (HG_TAB - 1), mine = EMPTY_SLOT;
                for (;;) {
                    u32 v = s_tab[h];
                    if (v == EMPTY_SLOT) {
                        if (mine == EMPTY_SLOT) {
                            mine = atomicAdd(&s_nkeys, 1u);
                            s_key[2 * mine] = key.lo;
                            s_key[2 * mine + 1] = key.hi;
                            s_cnt[mine] = 0;
                            __threadfence_block();  // the key is in place before the table points at it
                        }
                        v = atomicCAS(&s_tab[h], EMPTY_SLOT, mine);
                        if (v == EMPTY_SLOT) {
                            atomicAdd(&s_cnt[mine], mult | HG_LIVE);
                            break;
                        }
                    }
                    __threadfence_block();
                    if (s_key[2 * v] == key.lo && s_key[2 * v + 1] == key.hi) {
                        atomicAdd(&s_cnt[v], mult);
                        break;
                    }
                    h = (h + 1) & (HG_TAB - 1);
                }
            }
            __syncthreads();
            const u32 nkeys = s_nkeys;
            // ---- the partition's entries: the ones that are in the chunk take its multiplicity (mod 256; SAT: up to 255)
            for (u32 e = tid; e < n_exist; e += HG_THREADS) {
                const u128x ke = load_key(ix, off + e);
                const u64 klo = ke.lo, khi = ke.hi;
                u32 h = hash_key32(mk128(klo, khi)) & (HG_TAB - 1);
                for (;;) {
                    const u32 v = s_tab[h];
                    if (v == EMPTY_SLOT) break;
                    if (s_key[2 * v] == klo && s_key[2 * v + 1] == khi) {
                        const u32 m = atomicOr(&s_cnt[v], HG_EXIST) & HG_MULT;
                        ix.counts[off + e] = (uint8_t)count8<SAT>(ix.counts[off + e] + m);
                        break;
                    }
                    h = (h + 1) & (HG_TAB - 1);
                }
            }
            __syncthreads();
            // ---- the new ones: counted, given room (the partition moves at most once per batch), appended
            u32 mine_new = 0;
            for (u32 q = tid; q < nkeys; q += HG_THREADS) {
                const u32 cv = s_cnt[q];
                mine_new += (cv & HG_LIVE) && !(cv & HG_EXIST) ? 1u : 0u;
            }
            u32 n_new;
            (void)block_incl_scan(mine_new, s_wsum, &n_new);
            inst_left -= ninst;
            if (n_exist + n_new > cap) {
                const unsigned long long want = grow_cap(n_exist + n_new + inst_left);
                if (tid == 0) {
                    const unsigned long long got = atomicAdd(ix.cursor, want);
                    s_noff = got;
                    if (got + want > ix.arena_cap) {  // must not happen (the host reserves the bound): drop, flag
                        atomicOr(ix.err, 2u);
                        s_fail = 1;
                    }
                }
                __syncthreads();
                if (s_fail) {
                    failed = true;
                    break;
                }
                const unsigned long long noff = s_noff;
                for (u32 e = tid; e < n_exist; e += HG_THREADS) {
                    move_key(ix, noff + e, off + e);
                    ix.counts[noff + e] = ix.counts[off + e];
                }
                garbage += cap;
                cap = (u32)want;
                off = noff;
            }
            u32 done = 0;  // new entries of the rounds before this one
            for (u32 q0 = 0; q0 < nkeys; q0 += HG_THREADS) {
                const u32 q = q0 + tid;
                const u32 cv = q < nkeys ? s_cnt[q] : 0;
                const bool is_new = (cv & HG_LIVE) && !(cv & HG_EXIST);
                u32 round;
                const u32 pos = block_incl_scan(is_new ? 1u : 0u, s_wsum, &round);
                if (is_new) {
                    const unsigned long long at = off + n_exist + done + pos - 1;
                    const u64 klo = s_key[2 * q], khi = s_key[2 * q + 1];
                    store_key(ix, at, klo, khi);
                    ix.counts[at] = (uint8_t)count8<SAT>(cv & HG_MULT);
                    // bucket id inside the partition: the key's top `shift` bits (<= 6 of them used here), as insert_body has it
                    const u32 bl = P.shift ? ((u32)shr128(mk128(klo, khi), kbits).lo & ((1u << P.shift) - 1)) : 0;
                    const u32 bb = P.shift > 6 ? (bl >> (P.shift - 6)) : bl;
                    atomicOr(&s_bm[bb >> 5], 1u << (bb & 31));
                }
                done += round;
            }
            n_exist += n_new;
            rc += nrec;
            __syncthreads();  // the table and the key store are reused by the next chunk
        }
        __syncthreads();
        if (tid == 0 && !failed) {
            ix.dir[d.part] = DirEnt{off, n_exist, cap};
            if (garbage) atomicAdd(&ix.stats[3], garbage);
        }
        if (P.shift <= 6 && tid < 2 && !failed) {  // bucket occupancy bits, as in insert_body's epilogue
            const u32 mask = s_bm[tid];
            const u32 nb = 1u << P.shift;
            const u64 first = ((u64)d.part << P.shift) >> P.ext_bits;
            if (mask) {
                if (nb >= 32) {
                    if (tid * 32 < nb) atomicOr(&ix.bucket_bits[(first >> 5) + tid], mask);
                } else if (tid == 0) {
                    atomicOr(&ix.bucket_bits[first >> 5], mask << (first & 31));
                }
            }
        }
        __syncthreads();
    }
}
