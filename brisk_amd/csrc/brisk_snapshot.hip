// brisk_snapshot.hip -- index snapshots: the live entries of a range of partitions to and from a dense buffer (k_snapshot_move),
// and the directory lines of a loaded block (k_snapshot_dir).  Included by brisk_kernels.hip (one translation unit).
// No reference counterpart (the reference's index lives as long as its process; jellyfish and KMC keep theirs on disk).
// ===========================================================================
// An entry's stored key plus its partition number is its whole identity (brisk_setops.hip), so a snapshot is the directory and the
// entries as stored: nothing is unhashed, scanned or inserted.  A block of the file is a list of
// (partition, count) pairs for its non-empty partitions and, dense and in that order, their keys and their counts.
//
// Pure data movement over runs of a dozen to a few thousand entries, so the work is shared out by DENSE POSITION, not by partition:
// a workgroup takes tiles of SNAP_TILE consecutive dense entries, a lane takes dense entry j, finds the pair whose run holds it and
// copies one key (8 or 16 bytes, one load and one store) and one count.  Every wave-instruction therefore moves 64 consecutive
// dense entries -- 1 KiB of two-word keys on the dense side, and on the arena side as many contiguous pieces as runs meet in those 64
// entries -- whatever the partition sizes are: 16 partitions of millions of entries (part_bits = 4) and millions of partitions of a
// dozen keep every lane of every wave busy alike, and a partition is never one wave's serial loop.
// Finding the pair: base[p] is the exclusive prefix of the pairs' counts (the host has the counts: it wrote, or has just read, the
// pairs).  tile_lo[t] is the pair that holds the first entry of tile t, also from the host, so no lane searches all of base[]:
// a lane bisects base[tile_lo[t] .. tile_lo[t + 1]] -- at working density (~76 entries a partition) 14 pairs, 4 steps that hit L1;
// one step fewer per halving of that, none inside a partition larger than a tile.
// GATHER (save): arena -> dense; the slice offsets come from the directory, which is only read.  Live entries only: a slice's
//   entries beyond cnt (after a prune or subtract) and abandoned slices are never reached.
// SCATTER (load with room): dense -> arena at arena_off[p], the offsets the host gave the new slices.
#define SNAP_TILE 1024u  // dense entries per tile: 4 per lane of a 256-lane workgroup

// the last p in [lo, hi] with base[p] <= j (base[lo] <= j is given)
__device__ __forceinline__ u32 snap_find(const u64* __restrict__ base, u32 lo, u32 hi, u64 j) {
    while (lo < hi) {
        const u32 mid = (lo + hi + 1) >> 1;
        if (base[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// pairs[p] = (partition, count) of the block's p-th non-empty partition; base[p] its first dense position; tile_lo[n_tiles + 1]
// with tile_lo[n_tiles] = n_pairs - 1; arena_off[p] (SCATTER only) the first arena entry of its new slice.
template <bool GATHER, u32 KW>
__global__ void __launch_bounds__(256) k_snapshot_move(IndexDev ix, const uint2* __restrict__ pairs, const u64* __restrict__ base, const u64* __restrict__ arena_off,
                                                       const u32* __restrict__ tile_lo, u32 n_pairs, u64 n_ent, u64* __restrict__ d_keys, uint8_t* __restrict__ d_counts) {
    const u64 n_tiles = (n_ent + SNAP_TILE - 1) / SNAP_TILE;
    for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const u32 lo = tile_lo[t], hi = min(tile_lo[t + 1], n_pairs - 1);
#pragma unroll
        for (u32 q = 0; q < SNAP_TILE / 256; q++) {
            const u64 j = t * SNAP_TILE + q * 256 + threadIdx.x;
            if (j >= n_ent) break;
            const u32 p = snap_find(base, lo, hi, j);
            const u64 e = j - base[p];
            if (e >= pairs[p].y) continue;  // (never: base is the prefix of the counts)
            const u64 at = (GATHER ? ix.dir[pairs[p].x].off : arena_off[p]) + e;
            if (at >= ix.arena_cap) continue;  // (never outside the arena)
            if (KW == 2) {
                ulonglong2* dense = reinterpret_cast<ulonglong2*>(d_keys) + j;
                ulonglong2* arena = reinterpret_cast<ulonglong2*>(ix.keys) + at;
                if (GATHER) *dense = *arena;
                else *arena = *dense;
            } else {
                if (GATHER) d_keys[j] = ix.keys[at];
                else ix.keys[at] = d_keys[j];
            }
            if (GATHER) d_counts[j] = ix.counts[at];
            else ix.counts[at] = d_counts[j];
        }
    }
}

// the directory lines of a loaded block: slice p starts at arena_off[p], holds pairs[p].y entries and has room for
// grow_cap of them (room != 0: a slice as the insert would have sized it) or for exactly them (compact)
__global__ void __launch_bounds__(256) k_snapshot_dir(DirEnt* __restrict__ dir, u32 n_parts, const uint2* __restrict__ pairs, const u64* __restrict__ arena_off, u32 n_pairs,
                                                      u32 room) {
    const u32 stride = gridDim.x * blockDim.x;
    for (u32 p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += stride) {
        const uint2 pr = pairs[p];
        if (pr.x >= n_parts) continue;  // (never: the host checked the pairs)
        DirEnt de;
        de.off = arena_off[p];
        de.cnt = pr.y;
        de.cap = room ? grow_cap(pr.y) : pr.y;
        dir[pr.x] = de;
    }
}
