// brisk_answers.hip -- the per-position get cut at the super-k-mer boundary (brisk_hip_record_kmers / _answer_records / _place_answers).
// Included by brisk_kernels.hip (one translation unit).
// ===========================================================================
// The owner of a bucket range does not hold the asker's slot array: it answers record i into a compact buffer, k-mer j of the record
// (the order its key is built in: minimizer_idx rising) at offsets[i] + j, and the asker moves every answer to its slot.  offsets =
// the exclusive prefix sum of the records' k-mer counts: both sides compute it from the records alone, so nothing but the records
// travels out and nothing but the answers travels back.

// ---- offsets: the records' k-mer counts scanned, 64-bit (2^32 - 1 records of up to 255 k-mers); k_slot_top scans the block sums ----
#define RECK_ITEMS 16
__device__ __forceinline__ u32 record_n(const BriskParams& P, const u64* __restrict__ rec, u64 i) { return hdr_n(rec[i * P.stride + P.nw]); }
__global__ void __launch_bounds__(256) k_reck_block(BriskParams P, const u64* __restrict__ rec, u64 n_rec, u64* __restrict__ block_sums) {
    __shared__ u64 s[4];
    const u64 base = (u64)blockIdx.x * 256 * RECK_ITEMS;
    u64 acc = 0;
    for (int i = 0; i < RECK_ITEMS; i++) {
        const u64 r = base + (u64)i * 256 + threadIdx.x;
        if (r < n_rec) acc += record_n(P, rec, r);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}
// offsets[i] for i < n_rec, and offsets[n_rec] = the total (written by the thread that holds the last record)
__global__ void __launch_bounds__(256) k_reck_apply(BriskParams P, const u64* __restrict__ rec, u64 n_rec, const u64* __restrict__ block_sums, u64* __restrict__ offsets) {
    __shared__ u64 s_wave[4];
    const u64 base = (u64)blockIdx.x * 256 * RECK_ITEMS + (u64)threadIdx.x * RECK_ITEMS;
    u32 n[RECK_ITEMS];
    u64 tsum = 0;
    for (int i = 0; i < RECK_ITEMS; i++) {
        n[i] = base + i < n_rec ? record_n(P, rec, base + i) : 0u;
        tsum += n[i];
    }
    u64 x = tsum;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(x, o, 64);
        if ((int)(threadIdx.x & 63) >= o) x += y;
    }
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = x;
    __syncthreads();
    u64 woff = 0;
    for (u32 j = 0; j < (threadIdx.x >> 6); j++) woff += s_wave[j];
    u64 run = block_sums[blockIdx.x] + woff + x - tsum;
    for (int i = 0; i < RECK_ITEMS; i++) {
        const u64 r = base + i;
        if (r >= n_rec) break;
        offsets[r] = run;
        run += n[i];
        if (r + 1 == n_rec) offsets[n_rec] = run;
    }
}

// ---- owner side: anchors under which the POS query kernels write k-mer j of record i to offsets[i] + j ----
// pos_slot0 turns a forward anchor a into a + idx0 - w: a = offsets[i] + w - idx0 (idx0 <= w, so nothing wraps; bit 63 stays clear: ascending)
__global__ void __launch_bounds__(256) k_answer_anchors(BriskParams P, const u64* __restrict__ rec, u64 n_rec, const u64* __restrict__ offsets, u64* __restrict__ anchors) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    const u32 idx0 = hdr_idx0(rec[i * P.stride + P.nw]) - P.suff_reduc;
    anchors[i] = offsets[i] + P.w - idx0;
}

// ---- asker side: answers[offsets[i] + j] -> the slot k_query<POS> would have written with the record's real anchor ----
// A wave takes 64 records: their answers are one contiguous stretch [offsets[r0], offsets[r0 + 64)), read 64 at a time; every lane
// finds its answer's record in the wave's 65 offsets (LDS) and stores to pos_slot(pos_slot0(anchor, idx0), j).  A slot outside the
// caller's n_slots is never stored: a broken anchor, flag 8 (pos_store's rule).
__global__ void __launch_bounds__(256) k_place_answers(BriskParams P, const u64* __restrict__ rec, const u32* __restrict__ tags, const u64* __restrict__ anchors, u64 n_rec,
                                                       const u64* __restrict__ offsets, const uint16_t* __restrict__ answers, uint16_t* __restrict__ slots, u64 n_slots,
                                                       u32* __restrict__ err) {
    __shared__ u64 s_off[4][65];
    __shared__ u64 s_s0[4][64];
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 n_groups = (n_rec + 63) / 64;
    for (u64 g = (u64)blockIdx.x * 4 + wv; g < n_groups; g += (u64)gridDim.x * 4) {
        const u64 r0 = g * 64, r = r0 + lane;
        const u32 cnt = (u32)min((u64)64, n_rec - r0);
        wave_sync();  // (the previous group's reads of the tables are done)
        if (lane < cnt) {
            s_off[wv][lane] = offsets[r];
            s_s0[wv][lane] = pos_slot0(P, anchors[tags[r]], hdr_idx0(rec[r * P.stride + P.nw]));
        }
        if (lane == 0) s_off[wv][cnt] = offsets[r0 + cnt];
        wave_sync();
        const u64 e0 = s_off[wv][0], e1 = s_off[wv][cnt];
        for (u64 e = e0 + lane; e < e1; e += 64) {
            u32 lo = 0, hi = cnt;  // the last record whose offset is <= e (records without k-mers are skipped by it)
            while (hi - lo > 1) {
                const u32 mid = (lo + hi) >> 1;
                if (s_off[wv][mid] <= e) lo = mid;
                else hi = mid;
            }
            pos_store(slots, n_slots, pos_slot(s_s0[wv][lo], (u32)(e - s_off[wv][lo])), answers[e], err);
        }
    }
}
