// brisk_graph.hip -- de Bruijn adjacency (brisk_hip_adjacency / _degree_spectrum / _prune_degrees): the eight possible neighbours of
// every entry, looked up on the device.  No reference counterpart (the reference answers for nodes only).  Included by brisk_capi.hip
// behind its last call: kernels first, then the host part and its own extern "C" block.
//
// Entry e has the string x: the k nucleotides of kmer_s as brisk_hip_enumerate unhashes it, leftmost nucleotide in the highest bits.
// Its neighbour strings are R_c = x[1:] + c (j = c) and L_c = c + x[:-1] (j = 4 + c), c = 0..3; bit j of the entry's adjacency byte
// is set when string j, looked up as a read of exactly k nucleotides (one brisk_hip_get_kmers slot), is present with a stored count
// >= min_count.  Self-loops, palindromes and an entry next to its own reverse complement need no rule: the lookup decides.
//
// k_neighbour_reads  the stored keys of a round's entries -> the packed stream of their 8 n reads of k nucleotides, starts[r] = r k
// k_fold_adjacency   the eight slots of an entry and the threshold -> its byte
// k_degree_hist      adjacency bytes and own counts -> the 26 bins of brisk_hip_degree_spectrum
// k_prune_degrees    k_prune with the predicate read from the entry's adjacency byte

#define GRAPH_BLOCK 256u
#define GRAPH_MAX_K 63u
#define GRAPH_CLASSES 26u

// the last partition p in [lo, hi] with gbase[p] <= t: gbase is the exclusive prefix of the directory counts, so empty partitions
// share their successor's base and the one found holds entry t
__device__ __forceinline__ u32 graph_part_of(const u64* __restrict__ gbase, u32 lo, u32 hi, u64 t) {
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        if (gbase[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One lane an entry, one block 256 consecutive entries of the round (entries [e0, e0 + n) of the index in enumeration order, in
// partitions [p_begin, p_begin + n_parts)).  Fused: the lane loads its key, undoes make_key and the compaction (entry_hashed_kmer),
// un-mixes the minimizer and builds the eight strings in registers; lo / hi never go through memory.
// The stream in 16-bit units: a read of k nucleotides is 2 k bits, an entry's eight reads are 16 k bits = k units, so entry t of the
// round owns units [t k, (t + 1) k) and a block's 256 entries own 128 k WHOLE words whatever the parity of k.  The lane cuts its
// strings into units (32 bits of a string at a time into a 64-bit accumulator: shifts by wave-uniform amounts, no division) and
// writes them to LDS -- distinct 16-bit addresses, so the word that an even and an odd entry share at odd k is put together
// there -- and then the block stores its words from LDS, each word once, by one lane, coalesced.  Unit g sits at LDS position g ^ 1:
// the earlier nucleotides are the word's high half.  The round's last block may end on half a word; its low half is zero.
// own_cnt[t]: the entry's own count byte (what the spectrum's node test reads), starts[r] = r k for r <= 8 n.
__global__ void __launch_bounds__(GRAPH_BLOCK) k_neighbour_reads(BriskParams P, IndexDev ix, const u64* __restrict__ gbase, u32 p_begin, u32 n_parts, u64 e0, u64 n,
                                                                 u32* __restrict__ packed, u64* __restrict__ starts, uint8_t* __restrict__ own_cnt) {
    __shared__ u32 s_words[GRAPH_BLOCK / 2 * GRAPH_MAX_K + 1];
    uint16_t* s16 = (uint16_t*)s_words;
    const u32 k = P.k, tid = threadIdx.x;
    const u64 b0 = (u64)blockIdx.x * GRAPH_BLOCK;  // < n
    const u32 nv = n - b0 < GRAPH_BLOCK ? (u32)(n - b0) : GRAPH_BLOCK;
    // the partitions of the block's first and last entry (block-uniform searches), then the lane's own between them
    const u32 q_lo = graph_part_of(gbase, p_begin, p_begin + n_parts - 1, e0 + b0);
    const u32 q_hi = graph_part_of(gbase, q_lo, p_begin + n_parts - 1, e0 + b0 + nv - 1);
    if (tid < nv) {
        const u64 t = b0 + tid;
        const u32 part = graph_part_of(gbase, q_lo, q_hi, e0 + t);
        const unsigned long long at = ix.dir[part].off + (e0 + t - gbase[part]);
        const u128x key = load_key(ix, at);
        own_cnt[t] = ix.counts[at];
        u32 idx;
        u128x x = entry_hashed_kmer(P, part, key, &idx);
        const u64 mm = mix2m_inv(shr128(x, 2 * idx).lo & P.m_mask, P.m_mask);  // unhash_kmer_minimizer (Kmers.cpp:178-187)
        x = or128(andn128(x, shl128(mk128(P.m_mask, 0), 2 * idx)), shl128(mk128(mm, 0), 2 * idx));
        const u128x r_base = and128(shl128(x, 2), mask128(2 * k)), l_base = shr128(x, 2);
        u64 acc = 0;
        u32 nbits = 0, g = tid * k;  // (j, left and nbits are the same in every lane: the loops are wave-uniform)
        for (u32 j = 0; j < 8; j++) {
            u128x s = j < 4 ? r_base : l_base;
            if (j < 4) s.lo |= j;
            else s = or128(s, shl128(mk128(j - 4, 0), 2 * (k - 1)));
            s = shl128(s, 128 - 2 * k);  // leftmost nucleotide in the top bits
            for (u32 left = 2 * k; left;) {
                const u32 len = left < 32 ? left : 32;
                acc = (acc << len) | (s.hi >> (64 - len));
                s = shl128(s, 32);
                nbits += len;
                left -= len;
                while (nbits >= 16) {
                    nbits -= 16;
                    s16[g ^ 1] = (uint16_t)(acc >> nbits);
                    g++;
                }
            }
        }
        for (u32 j = 0; j < 8; j++) starts[8 * t + j] = (8 * t + j) * (u64)k;
        if (t == n - 1) {
            starts[8 * n] = 8 * n * (u64)k;
            if ((nv * k) & 1) s16[(nv * k) ^ 1] = 0;
        }
    }
    __syncthreads();
    const u32 n_w = (nv * k + 1) / 2;
    u32* out = packed + b0 / 2 * k;
    for (u32 w = tid; w < n_w; w += GRAPH_BLOCK) out[w] = s_words[w];
}

// a slot of brisk_hip_get_kmers (0x100 | count where present, else 0) against the threshold
__device__ __forceinline__ u32 graph_pass(u32 slot, u32 min_count) { return (slot & 0x100u) && (slot & 0xffu) >= min_count; }

// slots[8 e + j]: neighbour j of the round's entry e (one 16-byte load a lane); adj[e]: its byte
__global__ void __launch_bounds__(256) k_fold_adjacency(const uint16_t* __restrict__ slots, u64 n, u32 min_count, uint8_t* __restrict__ adj) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint4 v = reinterpret_cast<const uint4*>(slots)[e];
    u32 a = 0;
    a |= graph_pass(v.x & 0xffffu, min_count) << 0 | graph_pass(v.x >> 16, min_count) << 1;
    a |= graph_pass(v.y & 0xffffu, min_count) << 2 | graph_pass(v.y >> 16, min_count) << 3;
    a |= graph_pass(v.z & 0xffffu, min_count) << 4 | graph_pass(v.z >> 16, min_count) << 5;
    a |= graph_pass(v.w & 0xffffu, min_count) << 6 | graph_pass(v.w >> 16, min_count) << 7;
    adj[e] = (uint8_t)a;
}

// the class of an entry: 5 * left + right for a node (own count >= min_count), 25 below the threshold
__device__ __forceinline__ u32 graph_class(u32 adj, u32 cnt, u32 min_count) {
    return cnt < min_count ? GRAPH_CLASSES - 1 : 5u * (u32)__popc(adj >> 4) + (u32)__popc(adj & 15u);
}

// out[c] += the entries of class c: one histogram per block in LDS, filled as k_spectrum fills its own (a real graph is (1, 1)
// almost everywhere: spectrum_add counts the lanes that want one bin with a ballot), one global atomic a non-empty bin and block
__global__ void __launch_bounds__(256) k_degree_hist(const uint8_t* __restrict__ adj, const uint8_t* __restrict__ own_cnt, u64 n, u32 min_count,
                                                     unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_hist[32];
    const u32 lane = threadIdx.x & 63;
    if (threadIdx.x < 32) s_hist[threadIdx.x] = 0;
    __syncthreads();
    for (u64 i0 = (u64)blockIdx.x * 256; i0 < n; i0 += (u64)gridDim.x * 256) {  // (block-uniform: every lane of a wave reaches the ballots)
        const u64 i = i0 + threadIdx.x;
        const bool valid = i < n;
        spectrum_add(s_hist, valid ? graph_class(adj[i], own_cnt[i], min_count) : 0u, valid, lane);
    }
    __syncthreads();
    if (threadIdx.x < GRAPH_CLASSES && s_hist[threadIdx.x]) atomicAdd(&out[threadIdx.x], s_hist[threadIdx.x]);
}

// k_prune (brisk_readout.hip) with another predicate: an entry goes when it is a node (count >= lo) of count <= hi whose class bit
// is set in class_mask; adj[gbase[part] + e] is the byte of entry e of the partition.  The ordering argument above k_prune holds
// as it stands: the predicate's two loads -- the count, as there, and the adjacency byte, from an array that this kernel never
// writes -- are issued by all lanes of a chunk before the ballot that its stores depend on; everything behind the ballot is k_prune's.
__global__ void __launch_bounds__(256) k_prune_degrees(IndexDev ix, u32 n_parts, const u64* __restrict__ gbase, const uint8_t* __restrict__ adj, u32 lo, u32 hi, u32 class_mask,
                                                       unsigned long long* __restrict__ removed_out) {
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6, lane = threadIdx.x & 63;
    unsigned long long removed = 0;  // wave-uniform
    for (u32 part = wave; part < n_parts; part += n_waves) {
        const DirEnt de = ix.dir[part];
        if (!de.cnt) continue;
        const u64 base = gbase[part];
        u32 written = 0;
        for (u32 e0 = 0; e0 < de.cnt; e0 += 64) {
            const u32 e = e0 + lane;
            const bool valid = e < de.cnt;
            const u32 c = valid ? ix.counts[de.off + e] : 0u;
            const u32 a = valid ? adj[base + e] : 0u;
            const bool keep = valid && !(c >= lo && c <= hi && ((class_mask >> graph_class(a, c, lo)) & 1u));
            const unsigned long long bal = __ballot(keep);
            const u32 slot = written + (u32)__popcll(bal & lanes_below(lane));  // <= e
            if (keep && slot != e) {
                const u128x key = load_key(ix, de.off + e);
                store_key(ix, de.off + slot, key.lo, key.hi);
                ix.counts[de.off + slot] = (uint8_t)c;
            }
            written += (u32)__popcll(bal);
        }
        if (written != de.cnt) {
            if (lane == 0) ix.dir[part].cnt = written;
            removed += de.cnt - written;
        }
    }
    if (lane == 0 && removed) atomicAdd(removed_out, removed);
}

// ---- host ----
namespace {

// a round holds whole partitions of at most this many entries (a larger partition goes alone): BRISK_GRAPH_BATCH, a test hook
u64 graph_batch_entries() {
    static const u64 n = getenv("BRISK_GRAPH_BATCH") && atoll(getenv("BRISK_GRAPH_BATCH")) > 0 ? (u64)atoll(getenv("BRISK_GRAPH_BATCH")) : (1ull << 22);
    return n;
}

int graph_envelope(brisk_hip_index* h, const char* who) {
    if (h->P.n_owners > 1)
        return fail(h, BRISK_HIP_EINVAL, std::string(who) + " on a sharded index (n_owners > 1): an entry's neighbours live with other owners; the sharded route is a follow-up");
    if (h->entry_ids) return fail(h, BRISK_HIP_EINVAL, std::string(who) + " on an entry-id index: its DATA lives on the host");
    if (h->P.k > GRAPH_MAX_K) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": k above 63");
    return BRISK_HIP_OK;
}

// the index as it stands: cnt[p] the directory counts, h->graph_base <- their exclusive prefix (entry e of partition p is row
// gbase[p] + e of brisk_hip_enumerate), *total the entries
int graph_plan(brisk_hip_index* h, std::vector<u32>& cnt, std::vector<u64>& gbase, u64* total) {
    cnt.resize(h->n_parts);
    gbase.resize(h->n_parts);
    hipLaunchKernelGGL(k_dir_counts, dim3(nblocks(h->n_parts, 256)), dim3(256), 0, h->stream, h->ix.dir, h->n_parts, h->d_cur32);  // (d_cur32 is per-batch scratch, free between batches)
    if (int lrc = launch_check(h, "k_dir_counts")) return lrc;
    HIPCHK(h, hipMemcpyAsync(cnt.data(), h->d_cur32, h->n_parts * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    u64 t = 0;
    for (u64 p = 0; p < h->n_parts; p++) {
        gbase[p] = t;
        t += cnt[p];
    }
    *total = t;
    return BRISK_HIP_OK;
}

struct GraphPhases {  // device time of the three phases of a call's rounds, when the handle profiles (brisk_hip_profile_enable)
    std::vector<hipEvent_t> ev;
    bool on;
    brisk_hip_index* h;
    explicit GraphPhases(brisk_hip_index* h_) : on(h_->profiling), h(h_) {}
    void mark() {
        if (!on) return;
        hipEvent_t e;
        hipEventCreate(&e);
        hipEventRecord(e, h->stream);
        ev.push_back(e);
    }
    void resolve() {  // the stream is idle; four marks a round
        for (size_t i = 0; i + 3 < ev.size(); i += 4)
            for (int ph = 0; ph < 3; ph++) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, ev[i + ph], ev[i + ph + 1]) == hipSuccess) h->graph_ms[ph] += ms;
            }
    }
    ~GraphPhases() {
        for (hipEvent_t e : ev) hipEventDestroy(e);
    }
};

// The adjacency bytes of every entry, round by round: whole partitions of at most graph_batch_entries() entries, formed as
// brisk_hip_reallocate forms its rounds.  Per round: the neighbour reads into h->graph_reads ([starts, 8 n + 1][the stream]), their
// slots into h->graph_slots through kmers_packed_impl in slices of at most max_batch_reads reads (a read of k nucleotides has one
// slot: slot 8 e + j is neighbour j of the round's entry e), and the fold.  d_adj: the whole array (the round stores at its base
// offset), or null -- the bytes of a round then live in h->graph_radj until the next one.  d_hist: null, or the 26 bins that every
// round's bytes and own counts are added to.  The handle's lock is held; the work is queued, not awaited.
int graph_adjacency_impl(brisk_hip_index* h, u32 min_count, const std::vector<u32>& cnt, const std::vector<u64>& gbase, uint8_t* d_adj, unsigned long long* d_hist) {
    const u64 k = h->P.k, round_cap = graph_batch_entries();
    int rc;
    if ((rc = ensure(h, h->graph_base, h->n_parts * 8))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->graph_base.p, gbase.data(), h->n_parts * 8, hipMemcpyHostToDevice, h->stream));
    GraphPhases phases(h);
    for (u64 p = 0; p < h->n_parts;) {
        while (p < h->n_parts && cnt[p] == 0) p++;
        if (p >= h->n_parts) break;
        u64 n = 0, q = p;
        while (q < h->n_parts && (n == 0 || n + cnt[q] <= round_cap)) n += cnt[q++];
        const u64 n_reads = 8 * n, n_words = (n * k + 1) / 2;
        if (n_reads >= (1ull << 40) || nblocks(n, GRAPH_BLOCK) > 0x7fffffffu) return fail(h, BRISK_HIP_EINVAL, "adjacency: a partition of more entries than one round covers");
        const size_t off_packed = ((n_reads + 1) * 8 + 15) / 16 * 16;
        if ((rc = ensure(h, h->graph_reads, off_packed + (n_words + 4) * 4))) return rc;
        if ((rc = ensure(h, h->graph_slots, n_reads * 2))) return rc;
        if ((rc = ensure(h, h->graph_cnt, n))) return rc;
        if (!d_adj && (rc = ensure(h, h->graph_radj, n))) return rc;
        u64* d_st = (u64*)h->graph_reads.p;
        u32* d_pk = (u32*)((char*)h->graph_reads.p + off_packed);
        uint16_t* d_slots = (uint16_t*)h->graph_slots.p;
        uint8_t* d_round = d_adj ? d_adj + gbase[p] : (uint8_t*)h->graph_radj.p;
        phases.mark();
        HIPCHK(h, hipMemsetAsync(d_pk + n_words, 0, 16, h->stream));  // (the stream is readable two words past its last nucleotide)
        hipLaunchKernelGGL(k_neighbour_reads, dim3(nblocks(n, GRAPH_BLOCK)), dim3(GRAPH_BLOCK), 0, h->stream, h->P, h->ix, (const u64*)h->graph_base.p, (u32)p, (u32)(q - p), gbase[p], n, d_pk,
                           d_st, (uint8_t*)h->graph_cnt.p);
        if ((rc = launch_check(h, "k_neighbour_reads"))) return rc;
        phases.mark();
        HIPCHK(h, hipMemsetAsync(d_slots, 0, n_reads * 2, h->stream));
        for (u64 r0 = 0; r0 < n_reads; r0 += h->max_batch_reads) {
            const u64 nr = std::min<u64>(h->max_batch_reads, n_reads - r0);
            if ((rc = kmers_packed_impl(h, d_pk, d_st + r0, nr, d_slots + r0, nr))) return rc;
        }
        phases.mark();
        hipLaunchKernelGGL(k_fold_adjacency, dim3(nblocks(n, 256)), dim3(256), 0, h->stream, (const uint16_t*)d_slots, n, min_count, d_round);
        if ((rc = launch_check(h, "k_fold_adjacency"))) return rc;
        if (d_hist) {
            hipLaunchKernelGGL(k_degree_hist, dim3((u32)std::min<u64>(nblocks(n, 256), 2048)), dim3(256), 0, h->stream, (const uint8_t*)d_round, (const uint8_t*)h->graph_cnt.p, n, min_count, d_hist);
            if ((rc = launch_check(h, "k_degree_hist"))) return rc;
        }
        phases.mark();
        p = q;
    }
    if (phases.on) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        phases.resolve();
    }
    return BRISK_HIP_OK;
}

}  // namespace

extern "C" {

BRISK_API int brisk_hip_adjacency(brisk_hip_index* h, uint32_t min_count, uint8_t* d_adj, uint64_t cap, uint64_t* n_entries) {
    if (!h || !n_entries) return BRISK_HIP_EINVAL;
    if (int erc = graph_envelope(h, "adjacency")) return erc;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    std::vector<u32> cnt;
    std::vector<u64> gbase;
    u64 total = 0;
    int rc;
    if ((rc = graph_plan(h, cnt, gbase, &total))) return rc;
    *n_entries = total;
    if (cap < total) return fail(h, BRISK_HIP_ECAPACITY, "adjacency: " + std::to_string(total) + " entries, d_adj holds " + std::to_string(cap));
    if (!total) return BRISK_HIP_OK;
    if (!d_adj) return BRISK_HIP_EINVAL;
    h->graph_ms[0] = h->graph_ms[1] = h->graph_ms[2] = 0;
    if ((rc = graph_adjacency_impl(h, min_count, cnt, gbase, d_adj, nullptr))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return check_device_flags(h);
}

BRISK_API int brisk_hip_degree_spectrum(brisk_hip_index* h, uint32_t min_count, uint64_t out[26]) {
    if (!h || !out) return BRISK_HIP_EINVAL;
    if (int erc = graph_envelope(h, "degree_spectrum")) return erc;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    std::vector<u32> cnt;
    std::vector<u64> gbase;
    u64 total = 0;
    int rc;
    if ((rc = graph_plan(h, cnt, gbase, &total))) return rc;
    if ((rc = ensure(h, h->graph_hist, GRAPH_CLASSES * 8))) return rc;
    unsigned long long* d_hist = (unsigned long long*)h->graph_hist.p;
    HIPCHK(h, hipMemsetAsync(d_hist, 0, GRAPH_CLASSES * 8, h->stream));
    h->graph_ms[0] = h->graph_ms[1] = h->graph_ms[2] = 0;
    if (total && (rc = graph_adjacency_impl(h, min_count, cnt, gbase, nullptr, d_hist))) return rc;
    HIPCHK(h, hipMemcpyAsync(out, d_hist, GRAPH_CLASSES * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return check_device_flags(h);
}

BRISK_API int brisk_hip_prune_degrees(brisk_hip_index* h, uint32_t min_count, uint32_t max_count, uint32_t class_mask, uint64_t* removed) {
    if (!h) return BRISK_HIP_EINVAL;
    if (int erc = graph_envelope(h, "prune_degrees")) return erc;
    if (min_count > max_count) return fail(h, BRISK_HIP_EINVAL, "prune_degrees: min_count > max_count");
    if (class_mask >> (GRAPH_CLASSES - 1)) return fail(h, BRISK_HIP_EINVAL, "prune_degrees: class_mask has a bit above 24 (the classes are 5 * left + right, left and right 0..4)");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    if (removed) *removed = 0;
    if (!class_mask || min_count > 255) return BRISK_HIP_OK;  // no class, or no node (counts are bytes): nothing can go
    std::vector<u32> cnt;
    std::vector<u64> gbase;
    u64 total = 0;
    int rc;
    if ((rc = graph_plan(h, cnt, gbase, &total))) return rc;
    if (!total) return BRISK_HIP_OK;
    // the whole array first, over the index as it stands: two dead ends that touch are both judged by the graph before the call
    if ((rc = ensure(h, h->graph_adj, total))) return rc;
    h->graph_ms[0] = h->graph_ms[1] = h->graph_ms[2] = 0;
    if ((rc = graph_adjacency_impl(h, min_count, cnt, gbase, (uint8_t*)h->graph_adj.p, nullptr))) return rc;
    HIPCHK(h, zero_ctr(h, &h->d_ctr->result.w[0]));
    hipLaunchKernelGGL(k_prune_degrees, dim3((u32)std::min<u64>(nblocks(h->n_parts * 64, 256), 2048)), dim3(256), 0, h->stream, h->ix, (u32)h->n_parts, (const u64*)h->graph_base.p,
                       (const uint8_t*)h->graph_adj.p, min_count, std::min<u32>(max_count, 255u), class_mask, h->d_ctr->result.w);
    if ((rc = launch_check(h, "k_prune_degrees"))) return rc;
    return after_removal(h, removed);
}

BRISK_API int brisk_hip_graph_phase_ms(brisk_hip_index* h, double out[3]) {
    if (!h || !out) return BRISK_HIP_EINVAL;
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    for (int i = 0; i < 3; i++) out[i] = h->graph_ms[i];
    return BRISK_HIP_OK;
}

}  // extern "C"
