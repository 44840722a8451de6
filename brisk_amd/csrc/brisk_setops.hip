// brisk_setops.hip -- combining two indexes: intersect, subtract, compare (k_join), the joint count-window filter and the joint
// count spectrum (k_joint), and merge (k_entries_to_records).
// Included by brisk_kernels.hip (one translation unit).  No reference counterpart (kmc_tools / jellyfish merge are the usual tools).
// ===========================================================================
// Two indexes with the same (k, m, b) and the same partition layout route an identity (kmer_s, minimizer_idx) to the same
// partition number and store it as the same key bits ([routing id low bits | compacted k-mer | idx'], make_key): the join is
// partition p of one against partition p of the other and compares keys as stored.  Nothing is hashed back, unhashed or scanned.
//
// k_join<OP, KW>: one wave per partition, persistent waves (a grid-stride loop over the partitions).  `src`'s partition goes into
// an LDS table in chunks of JN_ENT entries, k_query_fast's table: the keys are distinct, so building compares nothing and a probe
// ends at the first match; a table word is [entry of the chunk | its count << 16].  `dst`'s entries probe it.
//
// A src partition of more than one chunk: a dst entry's match state has to live across chunks.  It lives in registers: the wave
// holds a BLOCK of JN_SUB x 64 dst entries (keys, counts, match words) and runs every table chunk past it before it goes on to the
// next block.  (The other way, a scratch byte per dst entry in device memory, builds every chunk once instead of once per
// block, but needs arena-sized scratch, a second pass over dst, and writes where this kernel only reads; with 256 entries a
// block a build of 256 entries stands against 256 probes, and the partitions this layout is made for -- a few dozen to a few
// hundred entries -- are one chunk and one or two blocks.)  With one chunk the table is built once for all blocks.
//
// INTERSECT / SUBTRACT compact the survivors in place, ranked by ballot, as k_prune does.  Why this is safe in place:
//  * every load of a block -- the keys and counts of its JN_SUB x 64 entries, by all lanes -- is issued, and its result used (the
//    probes compare the keys), before the first ballot of the block's compaction, which every store of the block follows.  A lane
//    stores the registers it loaded.  A survivor whose slot is its own index and whose count stays stores nothing;
//  * written never exceeds the block's first index and a survivor's slot never exceeds its own index, so a block's stores go to
//    entries of this block or below: never to the next block's entries, which are loaded later, and earlier blocks are never read again.
// A partition with nothing to remove and no count to change stores nothing at all: not the directory line either.
// COMPARE writes to neither index: per-lane sums, reduced over the wave once, then one global atomic per wave and output.
// No wave-wide atomic on one LDS word, no returning global atomic per element (findings 1 and 8).
#define JN_ENT 256u    // src entries per table chunk
#define JN_TAB 512u    // table slots (at most half full)
#define JN_SUB 4u      // sub-chunks of 64 dst entries a wave holds in registers
#define JOIN_INTERSECT 0u
#define JOIN_SUBTRACT 1u
#define JOIN_COMPARE 2u
#define JOIN_RULE_SUM_SAT 4u   // k_join's rule beyond BRISK_HIP_COUNT_*: SUM between two saturating indexes, min(255, dst + src)
#define JN_FOUND 0x100u   // match word: JN_FOUND | the src entry's count; 0: not found (a count of 0 is still found)

// one probe of the table by every lane that has `valid`: returns the match word
template <u32 KW>
__device__ __forceinline__ u32 join_probe(const u64* s_key, const u32* s_tab, u32 tmask, u128x key, bool valid) {
    u32 h = hash_key32(key) & tmask, found = 0;
    bool p = valid;
    while (__any(p)) {
        const u32 v = p ? s_tab[h] : EMPTY_SLOT;
        const u32 x = v == EMPTY_SLOT ? 0 : (v & 0xffffu);
        const u64 q0 = s_key[KW * x], q1 = KW == 2 ? s_key[KW * x + 1] : 0;
        if (p) {
            if (v == EMPTY_SLOT) p = false;
            else if (q0 == key.lo && q1 == key.hi) {
                found = JN_FOUND | (v >> 16);
                p = false;
            } else h = (h + 1) & tmask;
        }
    }
    return found;
}

// rule: BRISK_HIP_COUNT_LEFT / MIN / MAX / SUM, or JOIN_RULE_SUM_SAT (INTERSECT only).  out: INTERSECT / SUBTRACT out[0] += entries removed;
// COMPARE out[0..5] as brisk_hip_compare documents them (dst is a, src is b).
template <u32 OP, u32 KW>
__global__ void __launch_bounds__(64) k_join(IndexDev dst, IndexDev src, u32 n_parts, u32 rule, unsigned long long* __restrict__ out) {
    __shared__ u64 s_key[KW * JN_ENT];
    __shared__ u32 s_tab[JN_TAB];
    const u32 lane = threadIdx.x;
    unsigned long long removed = 0, n_a = 0, n_b = 0;         // wave-uniform
    unsigned long long l_both = 0, l_min = 0, l_a = 0, l_b = 0;  // per lane (COMPARE)
    for (u32 part = blockIdx.x; part < n_parts; part += gridDim.x) {
        const DirEnt dd = dst.dir[part], ds = src.dir[part];
        const u32 nd = dd.cnt, ns = ds.cnt;
        if (OP == JOIN_COMPARE) {
            n_a += nd;
            n_b += ns;
        }
        if (nd == 0) continue;
        if (ns == 0) {  // nothing is shared
            if (OP == JOIN_INTERSECT) {
                if (lane == 0) dst.dir[part].cnt = 0;
                removed += nd;
            }
            continue;
        }
        const u32 n_chunks = (ns + JN_ENT - 1) / JN_ENT;
        // (a small partition clears and probes a small table: at most half full, at least 64 slots)
        u32 tsize = JN_TAB;
        if (n_chunks == 1) {
            tsize = 64;
            while (tsize < 2 * ns) tsize <<= 1;
        }
        const u32 tmask = tsize - 1;
        u32 written = 0;
        for (u32 b0 = 0; b0 < nd; b0 += JN_SUB * 64) {
            u128x key[JN_SUB];
            u32 cnt[JN_SUB], mw[JN_SUB];
#pragma unroll
            for (u32 q = 0; q < JN_SUB; q++) {
                const u32 e = b0 + q * 64 + lane;
                key[q] = mk128(0, 0);
                cnt[q] = 0;
                mw[q] = 0;
                if (e < nd) {
                    key[q] = load_key<KW>(dst, dd.off + e);
                    cnt[q] = dst.counts[dd.off + e];
                }
            }
            for (u32 c = 0; c < n_chunks; c++) {
                if (n_chunks > 1 || b0 == 0) {
                    const u32 c0 = c * JN_ENT, ne = min(ns - c0, JN_ENT);
                    wave_sync();  // the previous chunk's probes are done
                    for (u32 i = lane; i < tsize; i += 64) s_tab[i] = EMPTY_SLOT;
                    wave_sync();
                    for (u32 e = lane; e < ne; e += 64) {
                        const u128x kv = load_key<KW>(src, ds.off + c0 + e);
                        s_key[KW * e] = kv.lo;
                        if (KW == 2) s_key[KW * e + 1] = kv.hi;
                        const u32 word = e | ((u32)src.counts[ds.off + c0 + e] << 16);
                        u32 h = hash_key32(kv) & tmask;
                        while (atomicCAS(&s_tab[h], EMPTY_SLOT, word) != EMPTY_SLOT) h = (h + 1) & tmask;
                    }
                    wave_sync();
                }
#pragma unroll
                for (u32 q = 0; q < JN_SUB; q++) {
                    if (b0 + q * 64 >= nd) break;  // wave-uniform
                    const bool open = b0 + q * 64 + lane < nd && !mw[q];
                    const u32 f = join_probe<KW>(s_key, s_tab, tmask, key[q], open);
                    if (f) mw[q] = f;
                }
            }
#pragma unroll
            for (u32 q = 0; q < JN_SUB; q++) {
                if (b0 + q * 64 >= nd) break;  // wave-uniform
                const u32 e = b0 + q * 64 + lane;
                const bool valid = e < nd, hit = mw[q] != 0;
                const u32 cs = mw[q] & 0xffu;
                if (OP == JOIN_COMPARE) {  // (per-lane sums: reduced once, at the end)
                    if (hit) {
                        l_both += 1;
                        l_a += cnt[q];
                        l_b += cs;
                        l_min += min(cnt[q], cs);
                    }
                } else {
                    const bool keep = valid && (OP == JOIN_INTERSECT ? hit : !hit);
                    u32 nc = cnt[q];
                    if (OP == JOIN_INTERSECT) nc = rule == 1 ? min(nc, cs) : rule == 2 ? max(nc, cs) : rule == 3 ? (nc + cs) & 0xffu : rule == JOIN_RULE_SUM_SAT ? min(nc + cs, 255u) : nc;
                    const unsigned long long bal = __ballot(keep);
                    const u32 slot = written + (u32)__popcll(bal & lanes_below(lane));  // <= e
                    if (keep && slot != e) store_key<KW>(dst, dd.off + slot, key[q].lo, key[q].hi);
                    if (keep && (slot != e || nc != cnt[q])) dst.counts[dd.off + slot] = (uint8_t)nc;
                    written += (u32)__popcll(bal);
                }
            }
        }
        if (OP != JOIN_COMPARE && written != nd) {
            if (lane == 0) dst.dir[part].cnt = written;
            removed += nd - written;
        }
    }
    if (OP == JOIN_COMPARE) {
        for (int o = 32; o > 0; o >>= 1) {
            l_both += __shfl_xor(l_both, o, 64);
            l_min += __shfl_xor(l_min, o, 64);
            l_a += __shfl_xor(l_a, o, 64);
            l_b += __shfl_xor(l_b, o, 64);
        }
        if (lane == 0) {
            if (l_both) atomicAdd(&out[0], l_both);
            if (n_a - l_both) atomicAdd(&out[1], n_a - l_both);
            if (n_b - l_both) atomicAdd(&out[2], n_b - l_both);
            if (l_min) atomicAdd(&out[3], l_min);
            if (l_a) atomicAdd(&out[4], l_a);
            if (l_b) atomicAdd(&out[5], l_b);
        }
    } else if (lane == 0 && removed) atomicAdd(out, removed);
}

// ---------------------------------------------------------------------------
// k_joint<OP, KW>: the joint count-window filter and the joint count spectrum.  A sibling of k_join, not two more OP values of
// it: the same pairing, chunks and register blocks, join_probe shared, k_join's text and instantiations untouched.
//
// JOINT_FILTER is INTERSECT's in-place compaction with another `keep`: a function of cnt[q], the match word and five
// wave-uniform window values.  The ordering argument written at k_join applies unchanged; no count is rewritten, so a
// survivor that keeps its slot stores nothing and a partition that loses nothing stores nothing.  ns == 0 means "every entry
// is absent from src": emptied without keep_absent, left alone under a full self window, else compacted on its counts.
//
// JOINT_SPECTRUM adds 1 to bin (sa, sb) per dst entry: sa its stored count, sb the matched src entry's stored count or
// BRISK_HIP_JOINT_ABSENT.  An ns == 0 partition walks the same code with no chunk: all its entries are (sa, absent).  Entries
// only in src are not seen here (match state is kept per dst entry): the caller takes that row from src's k_spectrum minus
// the matched column sums.  The matrix (257 x 257 x 8 B) does not fit LDS and real spectra put nearly everything into a
// handful of low bins, so an LDS tile of JS_TILE x JS_TILE 32-bit bins holds states 0..JS_T-1 and `absent` (column JS_T) of
// both axes.  A pass of 64 entries goes in by k_spectrum's leader ballot on the combined bin id: one lane adds the popcount
// of the lanes that share the first lane's bin, for JS_ROUNDS rounds or until JS_DIRECT lanes are left, which add 1 each; a
// bin outside the tile takes the same aggregated add in global memory, result unused (no returning atomic).
// The JS_WAVES waves of a block share ONE tile (each has its own table): 52 KB a block of two-word keys, 24 waves a CU, where
// a tile per wave (10 KB) allows 16 and k_join has 26.  The tile is flushed -- one global add per non-empty bin -- when the
// block ends, and by any wave that has added 2^28 entries since its last flush: a flush takes a bin with an exchange, so it
// may run beside the other waves' adds, and JS_WAVES x 2^28 bounds every bin below 2^32.
// What a pass costs is the instructions it issues (measured, DESIGN.md section 4.r: sharing the tile bought 9 %, taking the
// global-memory branch out of the common pass 35 %), hence joint_add_pass<ALL_IN>.
#define JOINT_FILTER 0u
#define JOINT_SPECTRUM 1u
#define JS_T 31u      // states 0..JS_T-1 are in the tile; mirrored by the tests
#define JS_TILE 32u   // tile edge: JS_T states and `absent`
#define JS_STATES 257u
#define JS_ABSENT 256u
#define JS_WAVES 8u   // waves of a JOINT_SPECTRUM block (JOINT_FILTER: one)
#define JS_FLUSH_AT (1u << 28)
#define JS_ROUNDS 4
#define JS_DIRECT 8
struct JointWindow {  // by value: wave-uniform.  Bounds as stored counts (<= 255); min_other > max_other: no present entry passes
    u32 min_self, max_self, min_other, max_other, keep_absent;
};

// One pass: every valid lane's entry into its bin.  v = sa << 9 | sb is what lanes are compared by, t the bin's tile slot where
// the bin is in the tile.  ALL_IN: every valid lane's bin is (wave-uniform; nearly every pass of a real spectrum): that body
// holds no global-memory code at all -- the kernel is bound by the instructions a pass issues, not by its loads.
template <bool ALL_IN>
__device__ __forceinline__ void joint_add_pass(u32* s_tile, unsigned long long* __restrict__ out, u32 v, u32 t, bool in_tile, bool valid, u32 lane) {
    unsigned long long left = __ballot(valid);  // wave-uniform
#pragma unroll
    for (int round = 0; round < JS_ROUNDS; round++) {
        if (__popcll(left) <= JS_DIRECT) break;
        const u32 first = (u32)__ffsll((long long)left) - 1;
        const u32 lead = (u32)__builtin_amdgcn_readlane((int)v, (int)first);
        const unsigned long long same = __ballot(valid && v == lead);
        if (lane == first) {  // (the leader holds the bin itself)
            if (ALL_IN || in_tile) atomicAdd(&s_tile[t], (u32)__popcll(same));
            else atomicAdd(&out[(v >> 9) * JS_STATES + (v & 0x1ffu)], (unsigned long long)__popcll(same));
        }
        valid = valid && v != lead;
        left &= ~same;
    }
    if (valid) {
        if (ALL_IN || in_tile) atomicAdd(&s_tile[t], 1u);
        else atomicAdd(&out[(v >> 9) * JS_STATES + (v & 0x1ffu)], 1ull);
    }
}
__device__ __forceinline__ void joint_add(u32* s_tile, unsigned long long* __restrict__ out, u32 sa, u32 sb, bool valid, u32 lane) {
    const bool in_tile = sa < JS_T && (sb < JS_T || sb == JS_ABSENT);
    const u32 v = (sa << 9) | sb, t = sa * JS_TILE + (sb == JS_ABSENT ? JS_T : sb);
    if (__ballot(valid && !in_tile) == 0) joint_add_pass<true>(s_tile, out, v, t, true, valid, lane);
    else joint_add_pass<false>(s_tile, out, v, t, in_tile, valid, lane);
}
// bins first, first + step, ... of the tile go to global memory; other waves may be adding meanwhile
__device__ __forceinline__ void joint_flush(u32* s_tile, unsigned long long* __restrict__ out, u32 first, u32 step) {
    for (u32 i = first; i < JS_TILE * JS_TILE; i += step) {
        if (!s_tile[i]) continue;
        const u32 n = atomicExch(&s_tile[i], 0u);
        const u32 sa = i / JS_TILE, tb = i % JS_TILE;
        if (n) atomicAdd(&out[sa * JS_STATES + (tb == JS_T ? JS_ABSENT : tb)], (unsigned long long)n);
    }
}

// out: JOINT_FILTER out[0] += entries removed; JOINT_SPECTRUM out[sa * 257 + sb] += dst entries in that bin (sa <= 255)
template <u32 OP, u32 KW>
__global__ void __launch_bounds__(OP == JOINT_SPECTRUM ? 64 * JS_WAVES : 64) k_joint(IndexDev dst, IndexDev src, u32 n_parts, JointWindow w, unsigned long long* __restrict__ out) {
    constexpr u32 WAVES = OP == JOINT_SPECTRUM ? JS_WAVES : 1;
    __shared__ u64 s_key_all[WAVES][KW * JN_ENT];
    __shared__ u32 s_tab_all[WAVES][JN_TAB];
    __shared__ u32 s_tile[OP == JOINT_SPECTRUM ? JS_TILE * JS_TILE : 1];
    const u32 lane = WAVES == 1 ? threadIdx.x : threadIdx.x & 63, wib = WAVES == 1 ? 0 : threadIdx.x >> 6;
    u64* const s_key = s_key_all[wib];
    u32* const s_tab = s_tab_all[wib];
    unsigned long long removed = 0;  // wave-uniform
    u32 in_tile = 0;                 // wave-uniform: entries this wave added since it last flushed
    if (OP == JOINT_SPECTRUM) {
        for (u32 i = threadIdx.x; i < JS_TILE * JS_TILE; i += 64 * WAVES) s_tile[i] = 0;
        __syncthreads();
    }
    for (u32 part = blockIdx.x * WAVES + wib; part < n_parts; part += gridDim.x * WAVES) {
        const DirEnt dd = dst.dir[part], ds = src.dir[part];
        const u32 nd = dd.cnt, ns = ds.cnt;
        if (nd == 0) continue;
        if (OP == JOINT_FILTER && ns == 0) {  // every entry is absent from src
            if (!w.keep_absent) {
                if (lane == 0) dst.dir[part].cnt = 0;
                removed += nd;
                continue;
            }
            if (w.min_self == 0 && w.max_self == 255) continue;
        }
        const u32 n_chunks = (ns + JN_ENT - 1) / JN_ENT;  // 0: nothing to probe
        u32 tsize = JN_TAB;
        if (n_chunks <= 1) {
            tsize = 64;
            while (tsize < 2 * ns) tsize <<= 1;
        }
        const u32 tmask = tsize - 1;
        u32 written = 0;
        for (u32 b0 = 0; b0 < nd; b0 += JN_SUB * 64) {
            if (OP == JOINT_SPECTRUM) {
                if (in_tile >= JS_FLUSH_AT) {
                    joint_flush(s_tile, out, lane, 64);
                    in_tile = 0;
                }
                in_tile += JN_SUB * 64;
            }
            u128x key[JN_SUB];
            u32 cnt[JN_SUB], mw[JN_SUB];
#pragma unroll
            for (u32 q = 0; q < JN_SUB; q++) {
                const u32 e = b0 + q * 64 + lane;
                key[q] = mk128(0, 0);
                cnt[q] = 0;
                mw[q] = 0;
                if (e < nd) {
                    if (OP == JOINT_FILTER || ns) key[q] = load_key<KW>(dst, dd.off + e);  // (the spectrum of an ns == 0 partition reads counts only)
                    cnt[q] = dst.counts[dd.off + e];
                }
            }
            for (u32 c = 0; c < n_chunks; c++) {
                if (n_chunks > 1 || b0 == 0) {
                    const u32 c0 = c * JN_ENT, ne = min(ns - c0, JN_ENT);
                    wave_sync();  // the previous chunk's probes are done
                    for (u32 i = lane; i < tsize; i += 64) s_tab[i] = EMPTY_SLOT;
                    wave_sync();
                    for (u32 e = lane; e < ne; e += 64) {
                        const u128x kv = load_key<KW>(src, ds.off + c0 + e);
                        s_key[KW * e] = kv.lo;
                        if (KW == 2) s_key[KW * e + 1] = kv.hi;
                        const u32 word = e | ((u32)src.counts[ds.off + c0 + e] << 16);
                        u32 h = hash_key32(kv) & tmask;
                        while (atomicCAS(&s_tab[h], EMPTY_SLOT, word) != EMPTY_SLOT) h = (h + 1) & tmask;
                    }
                    wave_sync();
                }
#pragma unroll
                for (u32 q = 0; q < JN_SUB; q++) {
                    if (b0 + q * 64 >= nd) break;  // wave-uniform
                    const bool open = b0 + q * 64 + lane < nd && !mw[q];
                    const u32 f = join_probe<KW>(s_key, s_tab, tmask, key[q], open);
                    if (f) mw[q] = f;
                }
            }
#pragma unroll
            for (u32 q = 0; q < JN_SUB; q++) {
                if (b0 + q * 64 >= nd) break;  // wave-uniform
                const u32 e = b0 + q * 64 + lane;
                const bool valid = e < nd, hit = mw[q] != 0;
                const u32 cs = mw[q] & 0xffu;
                if (OP == JOINT_SPECTRUM) {
                    joint_add(s_tile, out, cnt[q], hit ? cs : JS_ABSENT, valid, lane);
                } else {
                    const bool keep = valid && cnt[q] >= w.min_self && cnt[q] <= w.max_self && (hit ? cs >= w.min_other && cs <= w.max_other : w.keep_absent != 0);
                    const unsigned long long bal = __ballot(keep);
                    const u32 slot = written + (u32)__popcll(bal & lanes_below(lane));  // <= e
                    if (keep && slot != e) {
                        store_key<KW>(dst, dd.off + slot, key[q].lo, key[q].hi);
                        dst.counts[dd.off + slot] = (uint8_t)cnt[q];
                    }
                    written += (u32)__popcll(bal);
                }
            }
        }
        if (OP == JOINT_FILTER && written != nd) {
            if (lane == 0) dst.dir[part].cnt = written;
            removed += nd - written;
        }
    }
    if (OP == JOINT_SPECTRUM) {
        __syncthreads();  // every wave of the block has left its loop
        joint_flush(s_tile, out, threadIdx.x, 64 * WAVES);
    } else if (lane == 0 && removed) atomicAdd(out, removed);
}

// ---------------------------------------------------------------------------
// merge: the entries of src's partitions [p_begin, p_begin + n_parts) become one-k-mer records for dst's insert, as
// brisk_hip_reallocate's records are -- but by a reshuffle of bits, without k_enumerate, reads or the scan: an entry's key IS
// make_key(routing id, compacted k-mer, idx'), and a record of one k-mer holds the compacted k-mer in its words and
// [routing id | n = 1 | idx' | multiplicity] in its header.  One lane per entry; the records leave in partition order, storage
// order inside one (out_base: the exclusive prefix of the partitions' sizes over the range).  The multiplicity is the stored
// count, HDR_HAS_MULT says it is there: a count of 0 arrives as 0, not as the 1 of a scanned record.
__global__ void __launch_bounds__(64) k_entries_to_records(BriskParams P, IndexDev src, u32 p_begin, u32 n_parts, const u64* __restrict__ out_base, u64 out_n,
                                                           u64* __restrict__ rec) {
    const u32 low_mask = (1u << P.shift) - 1;
    for (u32 pi = blockIdx.x; pi < n_parts; pi += gridDim.x) {
        const u32 part = p_begin + pi;
        const DirEnt de = src.dir[part];
        const u64 ob = out_base[pi];
        for (u32 e = threadIdx.x; e < de.cnt; e += 64) {
            if (ob + e >= out_n) break;  // (never outside the records' buffer)
            const u128x key = load_key(src, de.off + e);
            const u128x comp = and128(shr128(key, 6), mask128(2 * P.kb));
            u32 rid = part << P.shift;
            if (P.shift) rid |= (u32)shr128(key, 2 * P.kb + 6).lo & low_mask;
            u64* r = rec + (ob + e) * P.stride;
            r[0] = comp.lo;
            if (P.nw > 1) r[1] = comp.hi;
            if (P.nw > 2) r[2] = 0;
            if (P.nw > 3) r[3] = 0;
            r[P.nw] = rec_header(rid, 1, (u32)key.lo & 63u) | HDR_HAS_MULT | ((u64)src.counts[de.off + e] << 48);
        }
    }
}
// the histogram those records have (what k_part_hist would count): records in the low, k-mer instances in the high 32 bits
__global__ void __launch_bounds__(256) k_dir_to_hist(const DirEnt* __restrict__ dir, u32 p_begin, u32 n_parts, unsigned long long* __restrict__ hist) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_parts) return;
    const unsigned long long c = dir[p_begin + i].cnt;
    hist[p_begin + i] = c | (c << 32);
}
