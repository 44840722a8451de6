// brisk_split.hip -- read splitting (brisk_hip_solid_runs / brisk_hip_extract_fragments_packed / brisk_hip_split_*): a read is cut at
// its weak k-mers and every run of solid slots that is long enough becomes a fragment of its own.  No reference counterpart (Quake,
// BFC and khmer's trim-low-abund -V cut reads like this before assembly or a second count).  Included by brisk_kernels.hip, behind
// brisk_intake.hip: the runs are found by the intake's own passes.
//
// The slots of a batch (brisk_hip_get_kmers' uint16: 0 absent, 0x100 | count present) lie read after read, so "maximal runs of solid
// slots inside one read, at least s_min long, in input order" is the intake's question with a slot where it has a byte.  Only the mask
// pass differs: k_split_mask writes the intake's mask words (16 positions a lane, valid bits = solid) from slots, the read-start bits
// come from the slot offsets through k_intake_bounds, and k_intake_first / _reduce / _top / _spread / _count / _apply / _kept run over
// that mask as they are.  Positions are slot indices of the batch (the intake's a0 is 0).
//
// k_split_offsets     soff[r] = the first slot of read r, soff[n_reads] = the batch's slots: the read table the intake's passes take
// k_split_mask        per lane of 16 slots: which are solid (<true>: which are not: brisk_correct.hip); per block of INTAKE_BLOCK slots the last position at which a run can begin
// k_split_rows        a run {read, first slot i, s slots} -> the fragment {read + r0, start = i, len = s + k - 1}: one vector store a row
// k_split_frag_block  a caller's fragment table, per block of 4096 rows: the nucleotides, the first bad row flagged (count pass);
//                     k_slot_top (brisk_scan.hip) scans the block sums
// k_split_frag_apply  per row, in table order: where it starts in the output (out_starts), where in the source (src_pos): what
//                     k_extract_gather (brisk_extract.hip) takes, unchanged -- it does not ask whether two rows share a read

__global__ void __launch_bounds__(256) k_split_offsets(const u64* __restrict__ starts, const u64* __restrict__ slot_base, u64 n_reads, u64 n_slots, u64* __restrict__ soff) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    soff[r] = r < n_reads ? slot_base[r] + starts[r] : n_slots;
}

__device__ __forceinline__ u32 split_solid(u32 v, u32 solid_min) { return (v & 0x100u) != 0 && (v & 0xffu) >= solid_min; }
__device__ __forceinline__ u64 split_min16(u64 n) { return n < 16 ? n : 16; }

// mask[lane]: the read-start bits (<< 16, k_intake_bounds) stand; the valid bits are added.  carry[block]: as k_intake_mask leaves it.
// WEAK (brisk_correct.hip): the mask inverted over the slots that exist -- valid = not solid, and the runs are the weak runs.
template <bool WEAK>
__global__ void __launch_bounds__(256) k_split_mask(const uint16_t* __restrict__ slots, u64 n_slots, u32 solid_min, u32* __restrict__ mask, u64* __restrict__ carry) {
    __shared__ u64 s_last[4];
    const u64 lane = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 x0 = lane * 16;
    u32 valid = 0, exist = 0xffffu;  // exist: which of the lane's 16 positions are slots
    if (x0 + 16 <= n_slots && ((uintptr_t)slots & 15) == 0) {  // (a caller's slots are aligned as uint16 asks: 2 bytes)
        const uint4 a = reinterpret_cast<const uint4*>(slots + x0)[0], b = reinterpret_cast<const uint4*>(slots + x0)[1];
        const u32 w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 8; i++) valid |= (split_solid(w[i] & 0xffffu, solid_min) << (2 * i)) | (split_solid(w[i] >> 16, solid_min) << (2 * i + 1));
    } else {
        exist = x0 < n_slots ? 0xffffu >> (16 - (u32)split_min16(n_slots - x0)) : 0u;
        for (u32 i = 0; i < 16 && x0 + i < n_slots; i++) valid |= split_solid(slots[x0 + i], solid_min) << i;
    }
    if (WEAK) valid = ~valid & exist;
    const u32 bnd = mask[lane] >> 16;
    mask[lane] = valid | (bnd << 16);
    // where a run can begin: after a slot that is not solid, or at a read's first slot
    const u32 cutmask = ((~valid & 0xffffu) << 1) | bnd;
    u64 last = cutmask ? x0 + (31 - __clz(cutmask)) : 0;
    for (int o = 32; o > 0; o >>= 1) last = intake_max(last, __shfl_down(last, o, 64));
    if ((threadIdx.x & 63) == 0) s_last[threadIdx.x >> 6] = last;
    __syncthreads();
    if (threadIdx.x == 0) carry[blockIdx.x] = intake_max(intake_max(s_last[0], s_last[1]), intake_max(s_last[2], s_last[3]));
}

__device__ __forceinline__ void split_store_row(IntakeFragment* __restrict__ out, u64 read, u32 start, u32 len) {
    if (((uintptr_t)out & 15) == 0) {
        *reinterpret_cast<uint4*>(out) = uint4{(u32)read, (u32)(read >> 32), start, len};
    } else {  // (a caller's table is aligned as its u64 member asks: 8 bytes)
        reinterpret_cast<uint2*>(out)[0] = uint2{(u32)read, (u32)(read >> 32)};
        reinterpret_cast<uint2*>(out)[1] = uint2{start, len};
    }
}

// runs: k_intake_apply's rows over slot positions (len = the run's slots; s + k - 1 fits 32 bits: no read has 2^32 nucleotides)
__global__ void __launch_bounds__(256) k_split_rows(const IntakeFragment* __restrict__ runs, u64 n, u32 k, u64 r0, IntakeFragment* __restrict__ out) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const IntakeFragment f = runs[j];
    split_store_row(out + j, f.read + r0, f.start, f.len + k - 1);
}

#define SPLIT_ITEMS 16
// a row is bad when read >= n_reads, len == 0 or start + len is beyond the read (a read whose table entries descend holds nothing)
__device__ __forceinline__ bool split_row_ok(const IntakeFragment& f, const u64* __restrict__ starts, u64 n_reads) {
    if (f.read >= n_reads || f.len == 0) return false;
    const u64 s0 = starts[f.read], s1 = starts[f.read + 1];
    return s1 >= s0 && (u64)f.start + f.len <= s1 - s0;
}
// flags[0]: the first bad row (atomicMin; ~0 none)
__global__ void __launch_bounds__(256) k_split_frag_block(const IntakeFragment* __restrict__ frags, u64 n_frags, const u64* __restrict__ starts, u64 n_reads,
                                                          u64* __restrict__ bsum_nts, unsigned long long* __restrict__ flags) {
    __shared__ u64 s[4];
    const u64 base = (u64)blockIdx.x * 256 * SPLIT_ITEMS;
    u64 nts = 0;
    for (int i = 0; i < SPLIT_ITEMS; i++) {
        const u64 j = base + (u64)i * 256 + threadIdx.x;
        if (j >= n_frags) continue;
        const IntakeFragment f = frags[j];
        if (split_row_ok(f, starts, n_reads)) nts += f.len;
        else atomicMin(flags, (unsigned long long)j);
    }
    const u64 t = intake_block_sum(nts, s);
    if (threadIdx.x == 0) bsum_nts[blockIdx.x] = t;
}

// bsum_nts: exclusively scanned, the total at [gridDim.x].  The rows are valid here (the host has read the flag).
__global__ void __launch_bounds__(256) k_split_frag_apply(const IntakeFragment* __restrict__ frags, u64 n_frags, const u64* __restrict__ starts, const u64* __restrict__ bsum_nts,
                                                          u64* __restrict__ out_starts, u64* __restrict__ src_pos) {
    __shared__ u64 s_n[4];
    const u64 base = (u64)blockIdx.x * 256 * SPLIT_ITEMS + (u64)threadIdx.x * SPLIT_ITEMS;
    u64 t_nts = 0;
    for (int i = 0; i < SPLIT_ITEMS; i++)
        if (base + i < n_frags) t_nts += frags[base + i].len;
    u64 xn = t_nts;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 yn = __shfl_up(xn, o, 64);
        if ((int)(threadIdx.x & 63) >= o) xn += yn;
    }
    if ((threadIdx.x & 63) == 63) s_n[threadIdx.x >> 6] = xn;
    __syncthreads();
    u64 wn = 0;
    for (u32 j = 0; j < (threadIdx.x >> 6); j++) wn += s_n[j];
    u64 at = bsum_nts[blockIdx.x] + wn + xn - t_nts;  // the nucleotides of the rows before this lane's
    for (int i = 0; i < SPLIT_ITEMS; i++) {
        const u64 j = base + i;
        if (j >= n_frags) break;
        const IntakeFragment f = frags[j];
        out_starts[j] = at;
        src_pos[j] = starts[f.read] + f.start;
        at += f.len;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out_starts[n_frags] = bsum_nts[gridDim.x];
}
