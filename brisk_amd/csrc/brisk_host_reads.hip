// brisk_host_reads.hip -- the read-cleaning host layer, a part of brisk_capi.hip (included there, not a translation unit of its own):
// profile -> select -> extract -> intake -> pair decision.  Helpers in an anonymous namespace, then the entry points in one extern "C"
// block.  Every call that profiles reads walks them in batches of min(max_batch_reads, BRISK_PROFILE_BATCH) through one of two loops,
// profile_packed_batches (a stream on the device) and profile_host_batches (host reads).  A shared check takes the subject of its
// message from the caller: the messages are part of the interface.
namespace {

// ---- per-read abundance profiles (no reference counterpart; kernels: brisk_profile.hip) ----
static_assert(sizeof(brisk_hip_read_profile) == sizeof(ReadProfile) && offsetof(brisk_hip_read_profile, sum) == offsetof(ReadProfile, sum) &&
                  offsetof(brisk_hip_read_profile, run_len) == offsetof(ReadProfile, run_len) && offsetof(brisk_hip_read_profile, median_present) == offsetof(ReadProfile, median_present),
              "the kernels write the C-ABI's record");

// reads above this many slots are reduced in segments of that many: -DBRISK_PROFILE_SEG=<slots> or the environment, read once
#ifndef BRISK_PROFILE_SEG
#define BRISK_PROFILE_SEG 4096
#endif
u32 profile_seg() {
    static const u32 seg = [] {
        long v = BRISK_PROFILE_SEG;
        if (const char* e = getenv("BRISK_PROFILE_SEG")) v = atol(e);
        return (u32)std::min<long>(std::max<long>(v, 1), (long)PROFILE_SEG_MAX);
    }();
    return seg;
}
// a profile call's batches hold at most this many reads (and at most max_batch_reads): their slots are the call's device memory
u64 profile_batch_reads() {
    static const u64 n = getenv("BRISK_PROFILE_BATCH") && atoll(getenv("BRISK_PROFILE_BATCH")) > 0 ? (u64)atoll(getenv("BRISK_PROFILE_BATCH")) : (1ull << 24);
    return n;
}
u64 profile_batch_limit(const brisk_hip_index* h) { return std::min<u64>(h->max_batch_reads, profile_batch_reads()); }

// One batch: its slots into kout_tmp (zeroed; kmers_packed_impl exactly as brisk_hip_get_kmers runs it), then one record per read into
// d_out[0 .. n_reads).  n_slots: the batch's slots (count_kmers / host_slots).
// caller_slots (brisk_hip_profile_slots): the batch's slots are ext_slots, as the caller holds them; nothing is looked up, only the slot bases are made.
int profile_batch(brisk_hip_index* h, const u32* d_packed, const u64* d_starts, u64 n_reads, u64 n_slots, u32 solid_min, ReadProfile* d_out,
                  bool caller_slots = false, const uint16_t* ext_slots = nullptr) {
    int rc;
    const u32 seg = profile_seg();
    // what the table holds: reads that need segments, and a read too long for the record's 32-bit fields
    if ((rc = ensure(h, h->prof_plan, 64))) return rc;
    unsigned long long* d_ctr = (unsigned long long*)h->prof_plan.p;
    HIPCHK(h, hipMemsetAsync(d_ctr, 0, 64, h->stream));
    const u32 grid_reads = std::max<u32>(std::min<u32>(nblocks(n_reads, 256), 4096), 1);
    hipLaunchKernelGGL(k_profile_count_long, dim3(grid_reads), dim3(256), 0, h->stream, d_starts, n_reads, (u32)h->P.k, seg, d_ctr);
    if ((rc = launch_check(h, "k_profile_count_long"))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->h_ctr->prof, d_ctr, 24, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const u64 n_segs = h->h_ctr->prof[0], n_longs = h->h_ctr->prof[1];
    if (h->h_ctr->prof[2]) return fail(h, BRISK_HIP_EINVAL, "read_profile: a read of more than 2^32-1 slots does not fit the record");
    if (caller_slots) {
        if ((rc = slot_bases(h, d_starts, n_reads))) return rc;
    } else if (n_slots) {
        if ((rc = ensure(h, h->kout_tmp, n_slots * 2))) return rc;
        HIPCHK(h, hipMemsetAsync(h->kout_tmp.p, 0, n_slots * 2, h->stream));
        if ((rc = kmers_packed_impl(h, d_packed, d_starts, n_reads, (uint16_t*)h->kout_tmp.p, n_slots))) return rc;
    } else {  // nothing to look up; the records still need the table's slot bases (all zero slots: never read)
        if ((rc = ensure(h, h->slot_buf, (n_reads + 1) * 8))) return rc;
    }
    const uint16_t* d_slots = caller_slots ? ext_slots : (const uint16_t*)h->kout_tmp.p;
    const u64* d_slot_base = (const u64*)h->slot_buf.p;
    {
        ProfScope ps(h, S_PROFILE);
        const u32 grid = std::max<u32>((u32)std::min<u64>((n_reads + 3) / 4, 8192), 1);  // a wave per read, grid-stride
        hipLaunchKernelGGL(k_profile_reads, dim3(grid), dim3(256), 0, h->stream, d_slots, d_starts, d_slot_base, n_reads, (u32)h->P.k, solid_min, seg, d_out);
        if ((rc = launch_check(h, "k_profile_reads"))) return rc;
    }
    if (!n_longs) return BRISK_HIP_OK;
    // [64 bytes of counters][long reads][segments][partials]
    const size_t off_longs = 64, off_segs = off_longs + n_longs * sizeof(ProfileLong), off_part = (off_segs + n_segs * sizeof(ProfileSeg) + 15) / 16 * 16;
    if ((rc = ensure(h, h->prof_plan, off_part + n_segs * sizeof(ProfilePartial)))) return rc;
    char* b0 = (char*)h->prof_plan.p;
    d_ctr = (unsigned long long*)b0;
    HIPCHK(h, hipMemsetAsync(d_ctr, 0, 64, h->stream));  // (ensure may have moved the buffer)
    ProfileLong* d_longs = (ProfileLong*)(b0 + off_longs);
    ProfileSeg* d_segs = (ProfileSeg*)(b0 + off_segs);
    ProfilePartial* d_part = (ProfilePartial*)(b0 + off_part);
    ProfScope ps(h, S_PROFILE_LONG);
    hipLaunchKernelGGL(k_profile_plan, dim3(grid_reads), dim3(256), 0, h->stream, d_starts, n_reads, (u32)h->P.k, seg, d_ctr, d_longs, n_longs, d_segs, n_segs);
    if ((rc = launch_check(h, "k_profile_plan"))) return rc;
    hipLaunchKernelGGL(k_profile_segments, dim3((u32)std::min<u64>((n_segs + 3) / 4, 8192)), dim3(256), 0, h->stream, d_slots, d_starts, d_slot_base, (u32)h->P.k, solid_min, seg,
                       (const ProfileSeg*)d_segs, n_segs, d_part);
    if ((rc = launch_check(h, "k_profile_segments"))) return rc;
    hipLaunchKernelGGL(k_profile_fold, dim3((u32)std::min<u64>((n_longs + 3) / 4, 8192)), dim3(256), 0, h->stream, d_starts, (u32)h->P.k, seg, (const ProfileLong*)d_longs, n_longs,
                       (const ProfilePartial*)d_part, d_out);
    return launch_check(h, "k_profile_fold");
}

// The handle's lock is held, pending inserts are completed.  The internal batches of a packed stream: a batch's records go to dest(r0),
// then each(r0, n, records).  Nothing waits for the stream here: the caller ends with check_device_flags (read_profile_packed synchronises before it).
template <class Dest, class Each>
int profile_packed_batches(brisk_hip_index* h, const u32* d_packed, const u64* d_starts, u64 n_reads, u32 solid_min, Dest&& dest, Each&& each) {
    const u64 batch = profile_batch_limit(h);
    for (u64 r0 = 0; r0 < n_reads; r0 += batch) {
        const u64 nb = std::min<u64>(batch, n_reads - r0);
        u64 ns = 0;
        int rc;
        if ((rc = count_kmers(h, d_starts + r0, nb, &ns))) return rc;  // (EINVAL on a table that does not ascend)
        ReadProfile* d_prof = dest(r0);
        if ((rc = profile_batch(h, d_packed, d_starts + r0, nb, ns, solid_min, d_prof))) return rc;
        if ((rc = each(r0, nb, (const ReadProfile*)d_prof))) return rc;
    }
    return BRISK_HIP_OK;
}

// The same for host reads (checked by check_profile_offsets): a batch is uploaded and packed, its records go to prof_out, then
// each(r0, n, records), then the stream is waited for: the next batch's upload overwrites the packed stream that this one's kernels read.
template <class Each>
int profile_host_batches(brisk_hip_index* h, const char* bases, const uint64_t* offsets, u64 n_reads, u32 solid_min, Each&& each) {
    const u64 saved = h->max_batch_reads;
    h->max_batch_reads = profile_batch_limit(h);  // for_each_host_batch cuts by it; the handle's lock is held
    int rc = for_each_host_batch(h, bases, offsets, n_reads, [&](u64 r0, u64 nr) -> int {
        int rc2;
        if ((rc2 = ensure(h, h->prof_out, nr * sizeof(ReadProfile)))) return rc2;
        ReadProfile* d_prof = (ReadProfile*)h->prof_out.p;
        if ((rc2 = profile_batch(h, (const u32*)h->packed_tmp.p, (const u64*)h->starts_tmp.p, nr, host_slots(offsets, r0, r0 + nr, h->P.k), solid_min, d_prof))) return rc2;
        if ((rc2 = each(r0, nr, (const ReadProfile*)d_prof))) return rc2;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return BRISK_HIP_OK;
    });
    h->max_batch_reads = saved;
    return rc ? rc : check_device_flags(h);
}

// the read table of a host profile call; who: the subject of the second message (the first names none)
int check_profile_offsets(brisk_hip_index* h, const uint64_t* offsets, u64 n_reads, const char* who) {
    for (u64 r = 0; r < n_reads; r++) {
        if (offsets[r + 1] < offsets[r]) return fail(h, BRISK_HIP_EINVAL, "read offsets do not ascend (offsets[i + 1] < offsets[i])");
        if (offsets[r + 1] - offsets[r] >= PROFILE_MAX_SLOTS + h->P.k) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": a read of more than 2^32-1 slots does not fit the record");
    }
    return BRISK_HIP_OK;
}

// ---- read extraction: rule, gather, the composed calls (no reference counterpart; kernels: brisk_extract.hip) ----
static_assert(sizeof(brisk_hip_read_interval) == sizeof(ReadInterval) && offsetof(brisk_hip_read_interval, len) == offsetof(ReadInterval, len), "the kernels write the C-ABI's interval");
static_assert(BRISK_HIP_SELECT_SOLID_RUN == SELECT_SOLID_RUN && BRISK_HIP_SELECT_MEDIAN == SELECT_MEDIAN && BRISK_HIP_SELECT_PRESENT == SELECT_PRESENT, "the kernel's kinds are the header's");

int check_rule(brisk_hip_index* h, const brisk_hip_select_rule* rule, const char* who) {
    if (!rule) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": null rule");
    if (rule->struct_size < sizeof(brisk_hip_select_rule)) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": rule.struct_size is smaller than brisk_hip_select_rule");
    if (rule->kind > BRISK_HIP_SELECT_PRESENT) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": unknown rule.kind " + std::to_string(rule->kind));
    if (rule->lo > rule->hi) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": rule.lo " + std::to_string(rule->lo) + " is above rule.hi " + std::to_string(rule->hi));
    return BRISK_HIP_OK;
}
// the handle's lock is held; the rule is checked
int select_impl(brisk_hip_index* h, const ReadProfile* d_prof, u64 n_reads, const brisk_hip_select_rule* rule, ReadInterval* d_iv) {
    if (!n_reads) return BRISK_HIP_OK;
    hipLaunchKernelGGL(k_select_intervals, dim3(nblocks(n_reads, 256)), dim3(256), 0, h->stream, d_prof, n_reads, (u32)h->P.k, rule->kind, std::max<u32>(rule->min_len, h->P.k), rule->lo,
                       rule->hi, d_iv);
    return launch_check(h, "k_select_intervals");
}

struct OutStream {  // one output stream: brisk_hip_extract_packed's d_out_packed, out_cap_words, d_out_starts, d_out_index
    u32* packed;
    u64 cap_words;
    u64* starts;
    u64* index;
};

// The handle's lock is held.  Counts and flags first (one pass over the table, a host synchronisation), then -- only when the
// intervals are valid and the output has room -- the tables of the kept reads and the gather: a refused call writes nothing.
int extract_impl(brisk_hip_index* h, const u32* d_packed, const u64* d_starts, u64 n_reads, const ReadInterval* d_iv, const OutStream& out, u64* n_out_reads, u64* n_out_nts) {
    int rc;
    *n_out_reads = *n_out_nts = 0;
    u64 n_out = 0, n_nts = 0;
    const u32 nb = nblocks(n_reads, 256 * EXT_ITEMS);
    u64 *d_bs_reads = nullptr, *d_bs_nts = nullptr;
    if (n_reads) {
        // [64 bytes of flags][block sums of kept reads, nb + 1][of kept nucleotides, nb + 1]
        if ((rc = ensure(h, h->ext_tmp, 64 + 2 * ((size_t)nb + 1) * 8))) return rc;
        unsigned long long* d_flags = (unsigned long long*)h->ext_tmp.p;
        d_bs_reads = (u64*)((char*)h->ext_tmp.p + 64);
        d_bs_nts = d_bs_reads + nb + 1;
        HIPCHK(h, hipMemsetAsync(d_flags, 0xff, 8, h->stream));
        HIPCHK(h, hipMemsetAsync(d_flags + 1, 0, 8, h->stream));
        hipLaunchKernelGGL(k_extract_block, dim3(nb), dim3(256), 0, h->stream, d_starts, d_iv, n_reads, d_bs_reads, d_bs_nts, d_flags);
        hipLaunchKernelGGL(k_slot_top, dim3(1), dim3(1024), 0, h->stream, d_bs_reads, nb);
        hipLaunchKernelGGL(k_slot_top, dim3(1), dim3(1024), 0, h->stream, d_bs_nts, nb);
        if ((rc = launch_check(h, "k_extract_block / k_slot_top"))) return rc;
        u64 got[4] = {0, 0, 0, 0};
        HIPCHK(h, hipMemcpyAsync(got, d_flags, 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(got + 2, d_bs_reads + nb, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(got + 3, d_bs_nts + nb, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (got[1]) return fail(h, BRISK_HIP_EINVAL, "extract_packed: read offsets do not ascend (offsets[i + 1] < offsets[i])");
        if (got[0] != ~0ull) return fail(h, BRISK_HIP_EINVAL, "extract_packed: the interval of read " + std::to_string(got[0]) + " ends beyond the read (start + len > its length)");
        n_out = got[2];
        n_nts = got[3];
    }
    *n_out_reads = n_out;
    *n_out_nts = n_nts;
    const u64 n_words = (n_nts + 15) / 16;
    if (out.cap_words < n_words + 2)
        return fail(h, BRISK_HIP_ECAPACITY, "extract_packed: " + std::to_string(n_nts) + " kept nucleotides need " + std::to_string(n_words + 2) + " words, out_cap_words is " + std::to_string(out.cap_words));
    if (!n_out) {  // nothing kept: the empty stream
        HIPCHK(h, hipMemsetAsync(out.starts, 0, 8, h->stream));
        HIPCHK(h, hipMemsetAsync(out.packed, 0, 8, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return BRISK_HIP_OK;
    }
    if ((rc = ensure(h, h->ext_src, n_out * 8))) return rc;
    hipLaunchKernelGGL(k_extract_apply, dim3(nb), dim3(256), 0, h->stream, d_starts, d_iv, n_reads, (const u64*)d_bs_reads, (const u64*)d_bs_nts, out.starts, out.index,
                       (u64*)h->ext_src.p);
    if ((rc = launch_check(h, "k_extract_apply"))) return rc;
    if (n_words + 2 > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, "extract_packed: more output words than one launch covers");
    hipLaunchKernelGGL(k_extract_gather<ExtractNoPatch>, dim3(nblocks(n_words + 2, 256)), dim3(256), 0, h->stream, d_packed, (const u64*)out.starts, (const u64*)h->ext_src.p, n_out, n_words, out.packed,
                       ExtractNoPatch{});
    if ((rc = launch_check(h, "k_extract_gather"))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

// ---- raw read intake: rule, passes, the host calls (clean_dna of counter.cpp:130-169 in bulk; kernels: brisk_intake.hip) ----
static_assert(sizeof(brisk_hip_fragment) == 16 && sizeof(IntakeFragment) == 16 && offsetof(brisk_hip_fragment, start) == offsetof(IntakeFragment, start) &&
                  offsetof(brisk_hip_fragment, len) == offsetof(IntakeFragment, len),
              "the kernels write the C-ABI's fragment");
static_assert(sizeof(brisk_hip_intake_rule) == 16 && sizeof(brisk_hip_intake_stats) == 64, "include/brisk_hip.h: 16 / 16 / 64 bytes");
static_assert(BRISK_HIP_INTAKE_BLOCK == INTAKE_BLOCK, "the header names the kernels' block");

// *min_len: the effective one, max(rule.min_len, k); *thr: 0 for no quality cut, else qual_base + min_qual
int check_intake_rule(brisk_hip_index* h, const brisk_hip_intake_rule* rule, bool have_quals, const char* who, u32* min_len, u32* thr) {
    if (!rule) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": null rule");
    if (rule->struct_size < sizeof(brisk_hip_intake_rule)) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": rule.struct_size is smaller than brisk_hip_intake_rule");
    if (rule->min_qual > 93) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": rule.min_qual " + std::to_string(rule->min_qual) + " is above 93");
    if (rule->qual_base != 0 && rule->qual_base != 33 && rule->qual_base != 64) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": rule.qual_base is " + std::to_string(rule->qual_base) + ", not 33 or 64");
    if (rule->min_qual && !have_quals) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": rule.min_qual > 0 needs the qualities");
    *min_len = std::max<u32>(rule->min_len, h->P.k);
    *thr = rule->min_qual ? (rule->qual_base ? rule->qual_base : 33u) + rule->min_qual : 0u;
    return BRISK_HIP_OK;
}

// The handle's lock is held; the rule is checked.  The table is checked and the counts are taken first (two host synchronisations),
// the fragment rows go to scratch (ink_tab: rows, then starts, then source positions), and only when the caller's room suffices
// are they copied out and the stream gathered: a refused call writes nothing.  d_out_starts == NULL (the host calls): the rows stay
// in scratch.  d_bases / d_quals are indexed by the table's offsets; neither is read outside [offsets[0], offsets[n_reads]).
int intake_impl(brisk_hip_index* h, const uint8_t* d_bases, const uint8_t* d_quals, const u64* d_offsets, u64 n_reads, u32 min_len, u32 thr, u32* d_out, u64 cap_words,
                u64* d_out_starts, IntakeFragment* d_out_frags, u64 frag_cap, brisk_hip_intake_stats* st) {
    int rc;
    memset(st, 0, sizeof(*st));
    st->n_reads = n_reads;
    // (k >= 5 on every handle that create accepts; the gather's LDS stage is sized by this bound)
    if (min_len < INTAKE_MIN_LEN) return fail(h, BRISK_HIP_EUNSUPPORTED, "intake: fragments of fewer than " + std::to_string(INTAKE_MIN_LEN) + " nucleotides");
    u64 lo = 0, hi = 0, a0 = 0, n_lanes = 0;
    u32 nb = 0;
    u64 *d_carry = nullptr, *d_first = nullptr;
    if (n_reads) {
        if ((rc = ensure(h, h->ink_tmp, 64))) return rc;
        unsigned long long* d_flags = (unsigned long long*)h->ink_tmp.p;
        HIPCHK(h, hipMemsetAsync(d_flags, 0, 8, h->stream));
        if (n_reads > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, "intake: more reads than one launch covers");
        hipLaunchKernelGGL(k_intake_check, dim3(nblocks(n_reads, 256)), dim3(256), 0, h->stream, d_offsets, n_reads, d_flags);
        if ((rc = launch_check(h, "k_intake_check"))) return rc;
        u64 got[3] = {0, 0, 0};
        HIPCHK(h, hipMemcpyAsync(got, d_flags, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(got + 1, d_offsets, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(got + 2, d_offsets + n_reads, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (got[0] & 1) return fail(h, BRISK_HIP_EINVAL, "intake: read offsets do not ascend (offsets[i + 1] < offsets[i])");
        if (got[0] & 2) return fail(h, BRISK_HIP_EINVAL, "intake: a read of 2^32 bytes or more does not fit the fragment record");
        lo = got[1];
        hi = got[2];
        st->n_bases_in = hi - lo;
    }
    if (hi > lo) {
        a0 = lo - ((uintptr_t)(d_bases + lo) & 15);  // (may wrap below zero: positions are taken relative to it, modulo 2^64)
        const u64 lo_x = lo - a0, hi_x = hi - a0;
        const u64 nb64 = (hi_x + INTAKE_BLOCK - 1) / INTAKE_BLOCK;
        if (nb64 > 0x7fffffffull) return fail(h, BRISK_HIP_EINVAL, "intake: more input blocks than one launch covers");
        nb = (u32)nb64;
        n_lanes = nb64 * 256;
        if ((rc = ensure(h, h->ink_mask, n_lanes * 4))) return rc;
        // [64 bytes of flags][the blocks' run begins, nb + 1][block sums: cut bases, cut qualities, fragments, nucleotides, short, nb + 1 each]
        // [the partials of the two-level scans, nb2 + 1 for each of the six]
        const u32 nb2 = nblocks(nb, INTAKE_SCAN);
        // [per block, nb + 1: the first read that starts in or behind it]
        if ((rc = ensure(h, h->ink_tmp, 64 + 7 * ((size_t)nb + 1) * 8 + 6 * ((size_t)nb2 + 1) * 8))) return rc;
        d_carry = (u64*)((char*)h->ink_tmp.p + 64);
        u64 *d_bs[5], *d_part[6];
        for (int i = 0; i < 5; i++) d_bs[i] = d_carry + (size_t)(i + 1) * (nb + 1);
        for (int i = 0; i < 6; i++) d_part[i] = d_carry + (size_t)6 * (nb + 1) + (size_t)i * (nb2 + 1);
        d_first = d_carry + (size_t)6 * (nb + 1) + (size_t)6 * (nb2 + 1);
        HIPCHK(h, hipMemsetAsync(h->ink_mask.p, 0, n_lanes * 4, h->stream));
        {
            ProfScope ps(h, S_INTAKE);
            hipLaunchKernelGGL(k_intake_bounds, dim3(nblocks(n_reads + 1, 256)), dim3(256), 0, h->stream, d_offsets, n_reads, a0, n_lanes, (u32*)h->ink_mask.p);
            hipLaunchKernelGGL(k_intake_first, dim3(nblocks((u64)nb + 1, 256)), dim3(256), 0, h->stream, d_offsets, n_reads, a0, (u64)nb, d_first);
            hipLaunchKernelGGL(k_intake_mask, dim3(nb), dim3(256), 0, h->stream, d_bases, d_quals, a0, lo_x, hi_x, thr, (u32*)h->ink_mask.p, d_carry, d_bs[0], d_bs[1]);
            hipLaunchKernelGGL(k_intake_reduce<true>, dim3(nb2), dim3(INTAKE_SCAN), 0, h->stream, (const u64*)d_carry, nb, d_part[5]);
            hipLaunchKernelGGL(k_intake_top, dim3(1), dim3(1024), 0, h->stream, d_part[5], nb2);
            hipLaunchKernelGGL(k_intake_spread<true>, dim3(nb2), dim3(INTAKE_SCAN), 0, h->stream, d_carry, nb, (const u64*)d_part[5]);
            hipLaunchKernelGGL(k_intake_count, dim3(nb), dim3(256), 0, h->stream, (const u32*)h->ink_mask.p, n_lanes, (const u64*)d_carry, min_len, d_bs[2], d_bs[3], d_bs[4]);
            for (int i = 0; i < 5; i++) {  // the totals of all five; the exclusive prefixes of the fragments and their nucleotides, which the apply pass takes
                hipLaunchKernelGGL(k_intake_reduce<false>, dim3(nb2), dim3(INTAKE_SCAN), 0, h->stream, (const u64*)d_bs[i], nb, d_part[i]);
                hipLaunchKernelGGL(k_slot_top, dim3(1), dim3(1024), 0, h->stream, d_part[i], nb2);
                if (i == 2 || i == 3) hipLaunchKernelGGL(k_intake_spread<false>, dim3(nb2), dim3(INTAKE_SCAN), 0, h->stream, d_bs[i], nb, (const u64*)d_part[i]);
            }
            if ((rc = launch_check(h, "k_intake_bounds / k_intake_first / k_intake_mask / k_intake_reduce / k_intake_top / k_intake_spread / k_intake_count / k_slot_top"))) return rc;
        }
        u64 tot[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < 5; i++) HIPCHK(h, hipMemcpyAsync(tot + i, d_part[i] + nb2, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        st->n_cut_base = tot[0];
        st->n_cut_qual = tot[1];
        st->n_fragments = tot[2];
        st->n_nts = tot[3];
        st->n_short = tot[4];
    }
    const u64 n_frag = st->n_fragments, n_words = (st->n_nts + 15) / 16;
    IntakeFragment* d_rows = nullptr;
    u64 *d_starts = nullptr, *d_src = nullptr;
    if (n_frag) {
        const u32 nbk = nblocks(n_frag, 256);
        const u32 nbk2 = nblocks(nbk, INTAKE_SCAN);
        if ((rc = ensure(h, h->ink_tab, n_frag * 16 + (n_frag + 1) * 8 + n_frag * 8 + ((size_t)nbk + 1) * 8 + ((size_t)nbk2 + 1) * 8))) return rc;
        d_rows = (IntakeFragment*)h->ink_tab.p;
        d_starts = (u64*)(d_rows + n_frag);
        d_src = d_starts + n_frag + 1;
        u64* d_kept = d_src + n_frag;
        const u64* d_bs_frag = d_carry + (size_t)3 * (nb + 1);
        const u64* d_bs_nts = d_carry + (size_t)4 * (nb + 1);
        {
            ProfScope ps(h, S_INTAKE);
            hipLaunchKernelGGL(k_intake_apply, dim3(nb), dim3(256), 0, h->stream, (const u32*)h->ink_mask.p, n_lanes, (const u64*)d_carry, min_len, d_bs_frag, d_bs_nts, d_offsets, n_reads, a0,
                               (const u64*)d_first, d_rows, d_starts, d_src);
            hipLaunchKernelGGL(k_intake_kept, dim3(nbk), dim3(256), 0, h->stream, (const IntakeFragment*)d_rows, n_frag, d_kept);
            u64* d_kept2 = d_kept + nbk + 1;
            hipLaunchKernelGGL(k_intake_reduce<false>, dim3(nbk2), dim3(INTAKE_SCAN), 0, h->stream, (const u64*)d_kept, nbk, d_kept2);
            hipLaunchKernelGGL(k_slot_top, dim3(1), dim3(1024), 0, h->stream, d_kept2, nbk2);
            if ((rc = launch_check(h, "k_intake_apply / k_intake_kept / k_intake_reduce / k_slot_top"))) return rc;
        }
        HIPCHK(h, hipMemcpyAsync(&st->n_reads_kept, d_kept + nbk + 1 + nbk2, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (frag_cap < n_frag)
        return fail(h, BRISK_HIP_ECAPACITY, "intake: " + std::to_string(n_frag) + " fragments, frag_cap is " + std::to_string(frag_cap));
    if (d_out && cap_words < n_words + 2)
        return fail(h, BRISK_HIP_ECAPACITY, "intake: " + std::to_string(st->n_nts) + " nucleotides need " + std::to_string(n_words + 2) + " words, out_cap_words is " + std::to_string(cap_words));
    if (!n_frag) {  // no fragment: the empty stream
        if (d_out_starts) HIPCHK(h, hipMemsetAsync(d_out_starts, 0, 8, h->stream));
        if (d_out) HIPCHK(h, hipMemsetAsync(d_out, 0, 8, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return BRISK_HIP_OK;
    }
    if (d_out_starts) HIPCHK(h, hipMemcpyAsync(d_out_starts, d_starts, (n_frag + 1) * 8, hipMemcpyDeviceToDevice, h->stream));
    if (d_out_frags) HIPCHK(h, hipMemcpyAsync(d_out_frags, d_rows, n_frag * 16, hipMemcpyDeviceToDevice, h->stream));
    if (d_out) {
        if (n_words + 2 > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, "intake: more output words than one launch covers");
        ProfScope ps(h, S_INTAKE);
        hipLaunchKernelGGL(k_intake_gather, dim3(nblocks(n_words + 2, 256)), dim3(256), 0, h->stream, d_bases, hi, (const u64*)d_starts, (const u64*)d_src, n_frag, n_words, d_out);
        if ((rc = launch_check(h, "k_intake_gather"))) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

// host reads -> the device, as they are, in pieces of whole reads (at least one) of about h->intake_piece bytes; body(r0, nr, d_bases,
// d_quals, d_offsets): the piece's table holds the caller's offsets, and the two pointers are displaced so that those index them;
// group: a piece holds a multiple of so many reads
template <class F>
int for_each_raw_piece(brisk_hip_index* h, const char* bases, const char* quals, const uint64_t* offsets, uint64_t n_reads, F&& body, u64 group = 1) {
    for (u64 r0 = 0; r0 < n_reads;) {
        const u64 r_hi = std::min<u64>(n_reads, r0 + (1ull << 26));
        u64 r1 = (u64)(std::upper_bound(offsets + r0, offsets + r_hi + 1, offsets[r0] + h->intake_piece) - offsets) - 1;
        if (group > 1) r1 = r0 + (r1 - r0) / group * group;  // (the pairs calls: whole pairs, n_reads a multiple of group)
        if (r1 <= r0) r1 = std::min<u64>(n_reads, r0 + group);
        const u64 nb = offsets[r1] - offsets[r0], nr = r1 - r0, pad = (nb + 15) & ~15ull;
        int rc;
        if ((rc = ensure(h, h->ink_raw, (quals ? 2 : 1) * pad + 16))) return rc;
        if ((rc = ensure(h, h->ink_offs, (nr + 1) * 8))) return rc;
        uint8_t* d_b = (uint8_t*)h->ink_raw.p;
        uint8_t* d_q = quals ? d_b + pad : nullptr;
        if (nb) {
            HIPCHK(h, hipMemcpyAsync(d_b, bases + offsets[r0], nb, hipMemcpyHostToDevice, h->stream));
            if (quals) HIPCHK(h, hipMemcpyAsync(d_q, quals + offsets[r0], nb, hipMemcpyHostToDevice, h->stream));
        }
        HIPCHK(h, hipMemcpyAsync(h->ink_offs.p, offsets + r0, (nr + 1) * 8, hipMemcpyHostToDevice, h->stream));
        if ((rc = body(r0, nr, (const uint8_t*)(d_b - offsets[r0]), quals ? (const uint8_t*)(d_q - offsets[r0]) : nullptr, (const u64*)h->ink_offs.p))) return rc;
        r0 = r1;
    }
    return BRISK_HIP_OK;
}

int check_raw_reads(brisk_hip_index* h, const uint64_t* offsets, uint64_t n_reads, const char* who) {
    for (u64 r = 0; r < n_reads; r++) {
        if (offsets[r + 1] < offsets[r]) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": read offsets do not ascend (offsets[i + 1] < offsets[i])");
        if (offsets[r + 1] - offsets[r] > 0xffffffffull) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": a read of 2^32 bytes or more does not fit the fragment record");
    }
    return BRISK_HIP_OK;
}
// *sum += x, field by field: brisk_hip_intake_stats and brisk_hip_pair_counts are 64-bit counters throughout
template <class T>
void add_counters(T* sum, const T& x) {
    static_assert(sizeof(T) % 8 == 0 && alignof(T) == 8, "a struct of 64-bit counters");
    uint64_t* a = (uint64_t*)sum;
    const uint64_t* b = (const uint64_t*)&x;
    for (size_t i = 0; i < sizeof(T) / 8; i++) a[i] += b[i];
}

// ---- paired-end reads: the pair decision over intervals, pairs and singles as two streams (no reference counterpart; khmer's
// extract-paired-reads and Trimmomatic's paired mode are the usual tools; kernels: brisk_pairs.hip).  Beside read extraction in
// purpose; behind the intake calls because the clean_pairs calls are built from both. ----
static_assert(sizeof(brisk_hip_pair_counts) == 64 && offsetof(brisk_hip_pair_counts, n_nts_pairs) == 40, "include/brisk_hip.h: eight 64-bit counters");
static_assert(BRISK_HIP_PAIR_EACH == PAIR_EACH && BRISK_HIP_PAIR_ALL == PAIR_ALL && BRISK_HIP_PAIR_ANY == PAIR_ANY, "the kernel's modes are the header's");

// h->pair_tab: [PAIR_CTR_ROWS rows of 64 bytes: k_pair_split's six counters, summed here][64 bytes: two flags][the intervals of intact pairs,
// n_reads][those of singles, n_reads]
constexpr size_t kPairCtrBytes = (size_t)PAIR_CTR_ROWS * 64, kPairHeadBytes = kPairCtrBytes + 64;
unsigned long long* pair_flags(brisk_hip_index* h) { return (unsigned long long*)((char*)h->pair_tab.p + kPairCtrBytes); }

int check_pairs(brisk_hip_index* h, u64 n_reads, u32 pair_mode, const char* who) {
    if (n_reads & 1) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": n_reads " + std::to_string(n_reads) + " is odd (an interleaved stream holds whole pairs)");
    if (pair_mode > BRISK_HIP_PAIR_ANY) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": unknown pair_mode " + std::to_string(pair_mode));
    if (n_reads / 2 > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": more pairs than one launch covers");
    return BRISK_HIP_OK;
}

// The handle's lock is held.  The table is checked first (a host synchronisation): a refused call writes nothing.
int fragment_intervals_impl(brisk_hip_index* h, const IntakeFragment* d_frags, u64 n_frags, u64 n_reads, ReadInterval* d_iv) {
    int rc;
    if (n_reads > 0x7fffffffull * 256 || n_frags > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, "fragment_intervals: more rows than one launch covers");
    if (n_frags) {
        if ((rc = ensure(h, h->pair_tab, kPairHeadBytes))) return rc;
        unsigned long long* d_flags = pair_flags(h);
        HIPCHK(h, hipMemsetAsync(d_flags, 0xff, 8, h->stream));
        hipLaunchKernelGGL(k_fragment_check, dim3(nblocks(n_frags, 256)), dim3(256), 0, h->stream, d_frags, n_frags, n_reads, d_flags);
        if ((rc = launch_check(h, "k_fragment_check"))) return rc;
        u64 bad = 0;
        HIPCHK(h, hipMemcpyAsync(&bad, d_flags, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (bad != ~0ull)
            return fail(h, BRISK_HIP_EINVAL, "fragment_intervals: row " + std::to_string(bad) + " of the fragment table names a read >= n_reads or stands before the row ahead of it (by read, then by position)");
    }
    if (!n_reads) return BRISK_HIP_OK;
    hipLaunchKernelGGL(k_fragment_intervals, dim3(nblocks(n_reads, 256)), dim3(256), 0, h->stream, d_frags, n_frags, n_reads, d_iv);
    return launch_check(h, "k_fragment_intervals");
}

// the handle's lock is held; n_reads and the mode are checked
int pair_intervals_impl(brisk_hip_index* h, const ReadInterval* d_each, const ReadInterval* d_whole, u64 n_reads, u32 pair_mode, ReadInterval* d_out) {
    if (!n_reads) return BRISK_HIP_OK;
    hipLaunchKernelGGL(k_pair_intervals, dim3(nblocks(n_reads / 2, 256)), dim3(256), 0, h->stream, d_each, d_whole, n_reads / 2, pair_mode, d_out);
    return launch_check(h, "k_pair_intervals");
}

// The handle's lock is held.  The inputs are checked first (a host synchronisation): a refused call writes nothing.
int compose_impl(brisk_hip_index* h, const ReadInterval* d_outer, u64 n_reads, const ReadInterval* d_inner, const u64* d_index, u64 n_kept, ReadInterval* d_out) {
    int rc;
    if (n_reads > 0x7fffffffull * 256 || n_kept > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, "compose_intervals: more rows than one launch covers");
    if (n_kept) {
        if ((rc = ensure(h, h->pair_tab, kPairHeadBytes))) return rc;
        unsigned long long* d_flags = pair_flags(h);
        HIPCHK(h, hipMemsetAsync(d_flags, 0xff, 16, h->stream));
        hipLaunchKernelGGL(k_compose_check, dim3(nblocks(n_kept, 256)), dim3(256), 0, h->stream, d_outer, n_reads, d_inner, d_index, n_kept, d_flags);
        if ((rc = launch_check(h, "k_compose_check"))) return rc;
        u64 got[2] = {0, 0};
        HIPCHK(h, hipMemcpyAsync(got, d_flags, 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (got[1] != ~0ull) return fail(h, BRISK_HIP_EINVAL, "compose_intervals: d_index does not ascend at row " + std::to_string(got[1]));  // (first: the rows of an index out of order pair the wrong intervals)
        if (got[0] != ~0ull)
            return fail(h, BRISK_HIP_EINVAL, "compose_intervals: row " + std::to_string(got[0]) + ": the inner interval leaves the outer one (start + len > outer.len), or d_index names a read >= n_reads");
    }
    if (!n_reads) return BRISK_HIP_OK;
    hipLaunchKernelGGL(k_compose_intervals, dim3(nblocks(n_reads, 256)), dim3(256), 0, h->stream, d_outer, n_reads, d_inner, d_index, n_kept, d_out);
    return launch_check(h, "k_compose_intervals");
}

// The handle's lock is held; n_reads is even.  The two masked tables into h->pair_tab, *counts filled.  d_starts (may be NULL: the
// intervals are then taken as they are): EINVAL where brisk_hip_extract_packed gives it, before anything is extracted.
int pair_split_impl(brisk_hip_index* h, const ReadInterval* d_iv, u64 n_reads, const u64* d_starts, brisk_hip_pair_counts* counts, const ReadInterval** iv_pairs,
                    const ReadInterval** iv_singles) {
    int rc;
    memset(counts, 0, sizeof(*counts));
    counts->n_pairs_in = n_reads / 2;
    *iv_pairs = *iv_singles = nullptr;
    if (!n_reads) return BRISK_HIP_OK;
    if ((rc = ensure(h, h->pair_tab, kPairHeadBytes + 2 * n_reads * sizeof(ReadInterval)))) return rc;
    unsigned long long* d_ctr = (unsigned long long*)h->pair_tab.p;
    unsigned long long* d_flags = pair_flags(h);
    ReadInterval* d_p = (ReadInterval*)((char*)h->pair_tab.p + kPairHeadBytes);
    ReadInterval* d_s = d_p + n_reads;
    HIPCHK(h, hipMemsetAsync(d_ctr, 0, kPairHeadBytes, h->stream));
    HIPCHK(h, hipMemsetAsync(d_flags, 0xff, 8, h->stream));
    hipLaunchKernelGGL(k_pair_split, dim3(nblocks(n_reads / 2, 256 * PAIR_ITEMS)), dim3(256), 0, h->stream, d_iv, n_reads / 2, d_starts, d_p, d_s, d_ctr, d_flags);
    if ((rc = launch_check(h, "k_pair_split"))) return rc;
    std::vector<u64> rows(kPairHeadBytes / 8);
    HIPCHK(h, hipMemcpyAsync(rows.data(), d_ctr, kPairHeadBytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    u64 got[8] = {0, 0, 0, 0, 0, 0, rows[kPairCtrBytes / 8], rows[kPairCtrBytes / 8 + 1]};
    for (size_t r = 0; r < PAIR_CTR_ROWS; r++)
        for (int i = 0; i < 6; i++) got[i] += rows[r * 8 + i];
    if (got[7]) return fail(h, BRISK_HIP_EINVAL, "extract_pairs_packed: read offsets do not ascend (offsets[i + 1] < offsets[i])");
    if (got[6] != ~0ull) return fail(h, BRISK_HIP_EINVAL, "extract_pairs_packed: the interval of read " + std::to_string(got[6]) + " ends beyond the read (start + len > its length)");
    counts->n_pairs_kept = got[0];
    counts->n_single_first = got[1];
    counts->n_single_second = got[2];
    counts->n_pairs_dropped = got[3];
    counts->n_nts_pairs = got[4];
    counts->n_nts_singles = got[5];
    *iv_pairs = d_p;
    *iv_singles = d_s;
    return BRISK_HIP_OK;
}

int check_pair_outs(brisk_hip_index* h, const OutStream& P, const OutStream& S, const brisk_hip_pair_counts* counts, const char* who) {
    if (!counts || !P.packed || !P.starts) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": null pointer");
    if (!S.packed || !S.starts) {
        if (S.packed || S.starts || S.index || S.cap_words) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": the singles output is given in part (all four NULL / 0 drops the singles)");
    }
    return BRISK_HIP_OK;
}

// The handle's lock is held; the arguments are checked.  Split and count (one pass, a host synchronisation), refuse before either
// stream is written, then brisk_hip_extract_packed's own block / apply / gather passes over each masked table.
int extract_pairs_impl(brisk_hip_index* h, const u32* d_packed, const u64* d_starts, u64 n_reads, const ReadInterval* d_iv, const OutStream& P, const OutStream& S,
                       brisk_hip_pair_counts* counts) {
    int rc;
    const ReadInterval *iv_p = nullptr, *iv_s = nullptr;
    if ((rc = pair_split_impl(h, d_iv, n_reads, d_starts, counts, &iv_p, &iv_s))) return rc;
    const u64 need_p = (counts->n_nts_pairs + 15) / 16 + 2, need_s = (counts->n_nts_singles + 15) / 16 + 2;
    if (P.cap_words < need_p)
        return fail(h, BRISK_HIP_ECAPACITY, "extract_pairs_packed: " + std::to_string(counts->n_nts_pairs) + " nucleotides of pairs need " + std::to_string(need_p) + " words, the pairs output holds " + std::to_string(P.cap_words));
    if (S.packed && S.cap_words < need_s)
        return fail(h, BRISK_HIP_ECAPACITY, "extract_pairs_packed: " + std::to_string(counts->n_nts_singles) + " nucleotides of singles need " + std::to_string(need_s) + " words, the singles output holds " + std::to_string(S.cap_words));
    u64 n_out = 0, n_nts = 0;
    if ((rc = extract_impl(h, d_packed, d_starts, n_reads, iv_p, P, &n_out, &n_nts))) return rc;
    if (n_out != 2 * counts->n_pairs_kept || n_nts != counts->n_nts_pairs) return fail(h, BRISK_HIP_EHIP, "extract_pairs_packed: the pairs stream and the pair counts disagree");
    if (!S.packed) return BRISK_HIP_OK;
    if ((rc = extract_impl(h, d_packed, d_starts, n_reads, iv_s, S, &n_out, &n_nts))) return rc;
    if (n_out != counts->n_single_first + counts->n_single_second || n_nts != counts->n_nts_singles) return fail(h, BRISK_HIP_EHIP, "extract_pairs_packed: the singles stream and the pair counts disagree");
    return BRISK_HIP_OK;
}

// A batch's records through the rule into d_each, and (d_whole given) through the rule that keeps a read whole, subject to the same
// minimum length: what BRISK_HIP_PAIR_ANY restores.
int select_batch(brisk_hip_index* h, const ReadProfile* d_prof, u64 n_reads, const brisk_hip_select_rule* rule, ReadInterval* d_each, ReadInterval* d_whole) {
    if (int rc = select_impl(h, d_prof, n_reads, rule, d_each)) return rc;
    if (!d_whole) return BRISK_HIP_OK;
    const brisk_hip_select_rule whole = {sizeof(whole), BRISK_HIP_SELECT_MEDIAN, rule->min_len, 0, 0xffffffffu};  // (a median is at most 255: every read with a k-mer passes)
    return select_impl(h, d_prof, n_reads, &whole, d_whole);
}

// The handle's lock is held, pending inserts are completed.  d_each[0 .. n_reads): the rule over the profiles of a packed stream, as
// brisk_hip_trim_packed computes them (profile_packed_batches, every batch into prof_out); d_whole (may be NULL): the same reads kept whole.
int profile_select(brisk_hip_index* h, const u32* d_packed, const u64* d_starts, u64 n_reads, u32 solid_min, const brisk_hip_select_rule* rule, ReadInterval* d_each,
                   ReadInterval* d_whole) {
    if (!n_reads) return BRISK_HIP_OK;
    if (int rc = ensure(h, h->prof_out, std::min<u64>(profile_batch_limit(h), n_reads) * sizeof(ReadProfile))) return rc;
    int rc = profile_packed_batches(h, d_packed, d_starts, n_reads, solid_min, [&](u64) { return (ReadProfile*)h->prof_out.p; },
                                    [&](u64 r0, u64 nb, const ReadProfile* d_prof) { return select_batch(h, d_prof, nb, rule, d_each + r0, d_whole ? d_whole + r0 : nullptr); });
    return rc ? rc : check_device_flags(h);
}

// The handle's lock is held; the rules and n_reads are checked; with a select rule pending inserts are completed.  Raw reads on the
// device -> *stats, and (n_reads > 0) out->intervals: one interval per raw read after the pair decision; out->raw / out->raw_starts: the raw
// bytes as a packed stream whose read table begins at 0 (scratch of the handle, all three).
struct CleanedPairs {
    const ReadInterval* intervals = nullptr;
    const u32* raw = nullptr;
    const u64* raw_starts = nullptr;
};
int clean_pairs_core(brisk_hip_index* h, const uint8_t* d_bases, const uint8_t* d_quals, const u64* d_offsets, u64 n_reads, u32 min_len, u32 thr,
                     const brisk_hip_select_rule* select, u32 solid_min, u32 pair_mode, brisk_hip_intake_stats* stats, CleanedPairs* out) {
    int rc;
    *out = CleanedPairs();
    if ((rc = intake_impl(h, d_bases, d_quals, d_offsets, n_reads, min_len, thr, nullptr, 0, nullptr, nullptr, ~0ull, stats))) return rc;  // the table only: its rows stay in ink_tab
    if (!n_reads) return BRISK_HIP_OK;
    if ((rc = ensure(h, h->pair_iv, 2 * n_reads * sizeof(ReadInterval)))) return rc;
    ReadInterval* d_iv1 = (ReadInterval*)h->pair_iv.p;
    ReadInterval* d_each = d_iv1 + n_reads;
    if ((rc = fragment_intervals_impl(h, (const IntakeFragment*)h->ink_tab.p, stats->n_fragments, n_reads, d_iv1))) return rc;
    // the raw bytes, packed: a byte that is no base packs to some code, and lies in no fragment
    u64 lo = 0;
    HIPCHK(h, hipMemcpyAsync(&lo, d_offsets, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const u64 n_bytes = stats->n_bases_in, n_words = (n_bytes + 15) / 16, words_room = (n_words + 3) & ~1ull;
    if ((rc = ensure(h, h->pair_raw, words_room * 4 + (n_reads + 1) * 8))) return rc;
    u32* d_packed = (u32*)h->pair_raw.p;
    u64* d_starts = (u64*)(d_packed + words_room);
    HIPCHK(h, hipMemsetAsync(d_packed + n_words, 0, 8, h->stream));
    if (n_words) {
        if (n_words > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, "clean_pairs: more input words than one launch covers");
        ProfScope ps(h, S_PACK);
        hipLaunchKernelGGL(k_pack_ascii, dim3(nblocks(n_words, 256)), dim3(256), 0, h->stream, d_bases + lo, n_bytes, d_packed, n_words);
    }
    hipLaunchKernelGGL(k_rebase_starts, dim3(nblocks(n_reads + 1, 256)), dim3(256), 0, h->stream, d_offsets, n_reads + 1, lo, d_starts);
    if ((rc = launch_check(h, "k_pack_ascii / k_rebase_starts"))) return rc;
    const ReadInterval* d_judged = d_iv1;
    if (select) {
        // the first longest fragment of every read as a stream of its own, its profile, the rule, and the cut back in the raw read's frame
        if ((rc = ensure(h, h->pair_fs, words_room * 4 + (n_reads + 1) * 8 + n_reads * 8))) return rc;
        u32* d_fs = (u32*)h->pair_fs.p;
        u64* d_fs_starts = (u64*)(d_fs + words_room);
        u64* d_fs_index = d_fs_starts + n_reads + 1;
        u64 n_kept = 0, n_nts = 0;
        if ((rc = extract_impl(h, d_packed, d_starts, n_reads, d_iv1, {d_fs, n_words + 2, d_fs_starts, d_fs_index}, &n_kept, &n_nts))) return rc;
        if ((rc = ensure(h, h->ext_iv, std::max<u64>(n_kept, 1) * sizeof(ReadInterval)))) return rc;
        if ((rc = profile_select(h, d_fs, d_fs_starts, n_kept, solid_min, select, (ReadInterval*)h->ext_iv.p, nullptr))) return rc;
        if ((rc = compose_impl(h, d_iv1, n_reads, (const ReadInterval*)h->ext_iv.p, d_fs_index, n_kept, d_each))) return rc;
        d_judged = d_each;
    }
    if ((rc = pair_intervals_impl(h, d_judged, d_iv1, n_reads, pair_mode, d_each))) return rc;
    *out = {d_each, d_packed, d_starts};
    return BRISK_HIP_OK;
}

int check_clean_pairs(brisk_hip_index* h, const brisk_hip_intake_rule* intake, bool have_quals, const brisk_hip_select_rule* select, u64 n_reads, u32 pair_mode, const char* who,
                      u32* min_len, u32* thr) {
    if (int rrc = check_intake_rule(h, intake, have_quals, who, min_len, thr)) return rrc;
    if (select) {
        if (int wrc = need_whole_index(h, std::string(who) + " with a select rule")) return wrc;
        if (int src = check_rule(h, select, who)) return src;
    }
    return check_pairs(h, n_reads, pair_mode, who);
}

// ---- read splitting: the solid runs of every read as fragments (no reference counterpart; kernels: brisk_split.hip over the
// intake's passes; the gather is brisk_extract.hip's) ----
static_assert(sizeof(brisk_hip_split_stats) == 64 && offsetof(brisk_hip_split_stats, n_nts_out) == 56, "include/brisk_hip.h: eight 64-bit counters");

// a run of s slots covers s + k - 1 nucleotides: at least max(min_len, k) of them when s >= this
u32 split_min_slots(const brisk_hip_index* h, u32 min_len) { return std::max<u32>(min_len, h->P.k) - h->P.k + 1; }

// The read table of a device call, checked as a whole (one pass, a host synchronisation); *n_nts: starts[n_reads] - starts[0].
// fit_record: a read whose nucleotides pass the fragment record's 32 bits is refused too.
int split_check_table(brisk_hip_index* h, const u64* d_starts, u64 n_reads, const char* who, bool fit_record, u64* n_nts) {
    int rc;
    if (n_reads > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": more reads than one launch covers");
    if ((rc = ensure(h, h->ink_tmp, 64))) return rc;
    unsigned long long* d_flags = (unsigned long long*)h->ink_tmp.p;
    HIPCHK(h, hipMemsetAsync(d_flags, 0, 8, h->stream));
    hipLaunchKernelGGL(k_intake_check, dim3(nblocks(n_reads, 256)), dim3(256), 0, h->stream, d_starts, n_reads, d_flags);
    if ((rc = launch_check(h, "k_intake_check"))) return rc;
    u64 got[3] = {0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(got, d_flags, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(got + 1, d_starts, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(got + 2, d_starts + n_reads, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (got[0] & 1) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": read offsets do not ascend (offsets[i + 1] < offsets[i])");
    if (fit_record && (got[0] & 2)) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": a read of 2^32 nucleotides or more does not fit the fragment record");
    *n_nts = got[2] - got[1];
    return BRISK_HIP_OK;
}

// The handle's lock is held.  One batch: d_slots[n_slots > 0] are the slots of the reads of d_starts[0 .. n_reads], and h->slot_buf
// holds their slot bases (slot_bases / kmers_packed_impl).  The intake's passes over a mask of solid slots: the counts first (a host
// synchronisation), then the runs {read, first slot, slots} into h->ink_tab, in input order, and *n_kept reads that have one.
// *run_slots: the slots of the runs of at least min_slots; *n_short: the solid slots of the shorter ones.
// weak (brisk_hip_weak_sites): the runs of slots that are NOT solid, over the same passes.
int split_runs_impl(brisk_hip_index* h, const uint16_t* d_slots, const u64* d_starts, u64 n_reads, u64 n_slots, u32 solid_min, u32 min_slots, u64* n_frag, u64* n_kept,
                    u64* run_slots, u64* n_short, bool weak = false) {
    int rc;
    *n_frag = *n_kept = *run_slots = *n_short = 0;
    const u64 nb64 = (n_slots + INTAKE_BLOCK - 1) / INTAKE_BLOCK;
    if (nb64 > 0x7fffffffull || n_reads > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, "split: more slots or reads than one launch covers");
    const u32 nb = (u32)nb64, nb2 = nblocks(nb, INTAKE_SCAN);
    const u64 n_lanes = nb64 * 256;
    if ((rc = ensure(h, h->split_off, (n_reads + 1) * 8))) return rc;
    if ((rc = ensure(h, h->ink_mask, n_lanes * 4))) return rc;
    // [the blocks' run begins, nb + 1][block sums: fragments, their slots, short, nb + 1 each][the partials of the two-level scans, nb2 + 1
    // for each of the four][per block, nb + 1: the first read that starts in or behind it]
    if ((rc = ensure(h, h->ink_tmp, (5 * ((size_t)nb + 1) + 4 * ((size_t)nb2 + 1)) * 8))) return rc;
    u64* d_soff = (u64*)h->split_off.p;
    u32* d_mask = (u32*)h->ink_mask.p;
    u64* d_carry = (u64*)h->ink_tmp.p;
    u64 *d_bs[3], *d_part[4];
    for (int i = 0; i < 3; i++) d_bs[i] = d_carry + (size_t)(i + 1) * (nb + 1);
    for (int i = 0; i < 4; i++) d_part[i] = d_carry + (size_t)4 * (nb + 1) + (size_t)i * (nb2 + 1);
    u64* d_first = d_carry + (size_t)4 * (nb + 1) + (size_t)4 * (nb2 + 1);
    HIPCHK(h, hipMemsetAsync(d_mask, 0, n_lanes * 4, h->stream));
    hipLaunchKernelGGL(k_split_offsets, dim3(nblocks(n_reads + 1, 256)), dim3(256), 0, h->stream, d_starts, (const u64*)h->slot_buf.p, n_reads, n_slots, d_soff);
    hipLaunchKernelGGL(k_intake_bounds, dim3(nblocks(n_reads + 1, 256)), dim3(256), 0, h->stream, (const u64*)d_soff, n_reads, (u64)0, n_lanes, d_mask);
    hipLaunchKernelGGL(k_intake_first, dim3(nblocks((u64)nb + 1, 256)), dim3(256), 0, h->stream, (const u64*)d_soff, n_reads, (u64)0, (u64)nb, d_first);
    if (weak) hipLaunchKernelGGL(k_split_mask<true>, dim3(nb), dim3(256), 0, h->stream, d_slots, n_slots, solid_min, d_mask, d_carry);
    else hipLaunchKernelGGL(k_split_mask<false>, dim3(nb), dim3(256), 0, h->stream, d_slots, n_slots, solid_min, d_mask, d_carry);
    hipLaunchKernelGGL(k_intake_reduce<true>, dim3(nb2), dim3(INTAKE_SCAN), 0, h->stream, (const u64*)d_carry, nb, d_part[3]);
    hipLaunchKernelGGL(k_intake_top, dim3(1), dim3(1024), 0, h->stream, d_part[3], nb2);
    hipLaunchKernelGGL(k_intake_spread<true>, dim3(nb2), dim3(INTAKE_SCAN), 0, h->stream, d_carry, nb, (const u64*)d_part[3]);
    hipLaunchKernelGGL(k_intake_count, dim3(nb), dim3(256), 0, h->stream, (const u32*)d_mask, n_lanes, (const u64*)d_carry, min_slots, d_bs[0], d_bs[1], d_bs[2]);
    for (int i = 0; i < 3; i++) {  // the totals of all three; the exclusive prefixes of the fragments and their slots, which the apply pass takes
        hipLaunchKernelGGL(k_intake_reduce<false>, dim3(nb2), dim3(INTAKE_SCAN), 0, h->stream, (const u64*)d_bs[i], nb, d_part[i]);
        hipLaunchKernelGGL(k_slot_top, dim3(1), dim3(1024), 0, h->stream, d_part[i], nb2);
        if (i < 2) hipLaunchKernelGGL(k_intake_spread<false>, dim3(nb2), dim3(INTAKE_SCAN), 0, h->stream, d_bs[i], nb, (const u64*)d_part[i]);
    }
    if ((rc = launch_check(h, "k_split_offsets / k_intake_bounds / k_intake_first / k_split_mask / k_intake_reduce / k_intake_top / k_intake_spread / k_intake_count / k_slot_top"))) return rc;
    u64 tot[3] = {0, 0, 0};
    for (int i = 0; i < 3; i++) HIPCHK(h, hipMemcpyAsync(tot + i, d_part[i] + nb2, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_frag = tot[0];
    *run_slots = tot[1];
    *n_short = tot[2];
    const u64 nf = tot[0];
    if (!nf) return BRISK_HIP_OK;
    if (nf > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, "split: more fragments than one launch covers");
    const u32 nbk = nblocks(nf, 256), nbk2 = nblocks(nbk, INTAKE_SCAN);
    // [rows][their starts in slots, nf + 1, and source positions, nf: k_intake_apply writes them, nothing reads them][kept reads per block of rows, and the partials]
    if ((rc = ensure(h, h->ink_tab, nf * 16 + (nf + 1) * 8 + nf * 8 + ((size_t)nbk + 1) * 8 + ((size_t)nbk2 + 1) * 8))) return rc;
    IntakeFragment* d_rows = (IntakeFragment*)h->ink_tab.p;
    u64* d_st = (u64*)(d_rows + nf);
    u64* d_src = d_st + nf + 1;
    u64* d_kept = d_src + nf;
    u64* d_kept2 = d_kept + nbk + 1;
    hipLaunchKernelGGL(k_intake_apply, dim3(nb), dim3(256), 0, h->stream, (const u32*)d_mask, n_lanes, (const u64*)d_carry, min_slots, (const u64*)d_bs[0], (const u64*)d_bs[1],
                       (const u64*)d_soff, n_reads, (u64)0, (const u64*)d_first, d_rows, d_st, d_src);
    hipLaunchKernelGGL(k_intake_kept, dim3(nbk), dim3(256), 0, h->stream, (const IntakeFragment*)d_rows, nf, d_kept);
    hipLaunchKernelGGL(k_intake_reduce<false>, dim3(nbk2), dim3(INTAKE_SCAN), 0, h->stream, (const u64*)d_kept, nbk, d_kept2);
    hipLaunchKernelGGL(k_slot_top, dim3(1), dim3(1024), 0, h->stream, d_kept2, nbk2);
    if ((rc = launch_check(h, "k_intake_apply / k_intake_kept / k_intake_reduce / k_slot_top"))) return rc;
    HIPCHK(h, hipMemcpyAsync(n_kept, d_kept2 + nbk2, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

// the runs in h->ink_tab as fragments of the call's reads (the batch begins at read r0), queued on the stream
int split_rows(brisk_hip_index* h, u64 n_frag, u64 r0, IntakeFragment* d_out) {
    hipLaunchKernelGGL(k_split_rows, dim3(nblocks(n_frag, 256)), dim3(256), 0, h->stream, (const IntakeFragment*)h->ink_tab.p, n_frag, (u32)h->P.k, r0, d_out);
    return launch_check(h, "k_split_rows");
}

// One batch of a composed call: its runs counted into *st and appended, as fragments, to the call's table in h->split_tab (which
// grows by copying: a call's table is small beside its reads).  st->n_fragments: the rows the table holds before the batch.
int split_batch(brisk_hip_index* h, const uint16_t* d_slots, const u64* d_starts, u64 n_reads, u64 n_slots, u64 r0, u32 solid_min, u32 min_slots, brisk_hip_split_stats* st) {
    int rc;
    st->n_slots += n_slots;
    if (!n_slots) return BRISK_HIP_OK;
    u64 nf = 0, kept = 0, run_slots = 0, n_short = 0;
    if ((rc = split_runs_impl(h, d_slots, d_starts, n_reads, n_slots, solid_min, min_slots, &nf, &kept, &run_slots, &n_short))) return rc;
    const u64 have = st->n_fragments;
    st->n_fragments += nf;
    st->n_reads_kept += kept;
    st->n_solid += run_slots + n_short;
    st->n_short += n_short;
    st->n_nts_out += run_slots + nf * (h->P.k - 1);
    if (!nf) return BRISK_HIP_OK;
    if (h->split_tab.bytes < (have + nf) * 16) {
        DevBuf grown;
        if ((rc = ensure(h, grown, std::max<size_t>((have + nf) * 16, 2 * h->split_tab.bytes)))) return rc;
        if (have) HIPCHK(h, hipMemcpyAsync(grown.p, h->split_tab.p, have * 16, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (h->split_tab.p) HIPCHK(h, hipFree(h->split_tab.p));
        h->split_tab = grown;
    }
    return split_rows(h, nf, r0, (IntakeFragment*)h->split_tab.p + have);
}

// The handle's lock is held.  The rows of a fragment table out of a packed stream: the rows checked and their nucleotides counted
// first (one pass, a host synchronisation), then -- only when the rows are valid and the output has room -- the starts, the source
// positions and brisk_hip_extract_packed's gather: a refused call writes nothing.  out.packed == NULL: the starts only.
// check_table: the read table is not known to ascend.
// cand_sites (brisk_hip_candidate_windows): the rows are the candidate windows of these sites, three a site, and the gather puts each
// candidate's substitution into its window.
int fragment_gather_impl(brisk_hip_index* h, const u32* d_packed, const u64* d_starts, u64 n_reads, const IntakeFragment* d_frags, u64 n_frags, const OutStream& out, bool check_table,
                         const char* who, u64* n_out_nts, const CorrectSite* cand_sites = nullptr) {
    int rc;
    *n_out_nts = 0;
    u64 n_nts = 0;
    if (check_table && n_reads) {
        u64 unused = 0;
        if ((rc = split_check_table(h, d_starts, n_reads, who, false, &unused))) return rc;  // (a long read is no fault here: rows address its first 2^32 nucleotides)
    }
    const u32 nb = nblocks(n_frags, 256 * SPLIT_ITEMS);
    u64* d_bs = nullptr;
    if (n_frags) {
        if (n_frags > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": more rows than one launch covers");
        // [64 bytes: the flag][block sums of the rows' nucleotides, nb + 1]
        if ((rc = ensure(h, h->ext_tmp, 64 + ((size_t)nb + 1) * 8))) return rc;
        unsigned long long* d_flags = (unsigned long long*)h->ext_tmp.p;
        d_bs = (u64*)((char*)h->ext_tmp.p + 64);
        HIPCHK(h, hipMemsetAsync(d_flags, 0xff, 8, h->stream));
        hipLaunchKernelGGL(k_split_frag_block, dim3(nb), dim3(256), 0, h->stream, d_frags, n_frags, d_starts, n_reads, d_bs, d_flags);
        hipLaunchKernelGGL(k_slot_top, dim3(1), dim3(1024), 0, h->stream, d_bs, nb);
        if ((rc = launch_check(h, "k_split_frag_block / k_slot_top"))) return rc;
        u64 got[2] = {0, 0};
        HIPCHK(h, hipMemcpyAsync(got, d_flags, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(got + 1, d_bs + nb, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (got[0] != ~0ull)
            return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": row " + std::to_string(got[0]) + " of the fragment table names a read >= n_reads, has len == 0, or ends beyond its read (start + len > its length)");
        n_nts = got[1];
    }
    *n_out_nts = n_nts;
    const u64 n_words = (n_nts + 15) / 16;
    if (out.packed && out.cap_words < n_words + 2)
        return fail(h, BRISK_HIP_ECAPACITY, std::string(who) + ": " + std::to_string(n_nts) + " nucleotides need " + std::to_string(n_words + 2) + " words, out_cap_words is " + std::to_string(out.cap_words));
    if (!n_frags) {  // no row: the empty stream
        HIPCHK(h, hipMemsetAsync(out.starts, 0, 8, h->stream));
        if (out.packed) HIPCHK(h, hipMemsetAsync(out.packed, 0, 8, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return BRISK_HIP_OK;
    }
    if ((rc = ensure(h, h->ext_src, n_frags * 8))) return rc;
    hipLaunchKernelGGL(k_split_frag_apply, dim3(nb), dim3(256), 0, h->stream, d_frags, n_frags, d_starts, (const u64*)d_bs, out.starts, (u64*)h->ext_src.p);
    if ((rc = launch_check(h, "k_split_frag_apply"))) return rc;
    if (out.packed) {
        if (n_words + 2 > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": more output words than one launch covers");
        const dim3 grid(nblocks(n_words + 2, 256));
        if (cand_sites)
            hipLaunchKernelGGL(k_extract_gather<CorrectCandPatch>, grid, dim3(256), 0, h->stream, d_packed, (const u64*)out.starts, (const u64*)h->ext_src.p, n_frags, n_words, out.packed,
                               CorrectCandPatch{cand_sites, (u32)h->P.k});
        else
            hipLaunchKernelGGL(k_extract_gather<ExtractNoPatch>, grid, dim3(256), 0, h->stream, d_packed, (const u64*)out.starts, (const u64*)h->ext_src.p, n_frags, n_words, out.packed,
                               ExtractNoPatch{});
        if ((rc = launch_check(h, "k_extract_gather"))) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

// ---- spectral read correction: isolated substitutions repaired (no reference counterpart; kernels: brisk_correct.hip over the
// split's run passes; the candidate windows are gathered by brisk_extract.hip's gather) ----
static_assert(sizeof(brisk_hip_correct_stats) == 88 && offsetof(brisk_hip_correct_stats, n_unresolved) == 80, "include/brisk_hip.h: eleven 64-bit counters");
static_assert(sizeof(brisk_hip_site) == sizeof(CorrectSite) && offsetof(brisk_hip_site, pos) == offsetof(CorrectSite, pos) && offsetof(brisk_hip_site, cover) == offsetof(CorrectSite, cover) &&
                  sizeof(brisk_hip_correction) == sizeof(CorrectRow) && offsetof(brisk_hip_correction, pos) == offsetof(CorrectRow, pos) &&
                  offsetof(brisk_hip_correction, from) == offsetof(CorrectRow, from) && offsetof(brisk_hip_correction, to) == offsetof(CorrectRow, to) &&
                  offsetof(brisk_hip_correction, cover) == offsetof(CorrectRow, cover),
              "the kernels write the C-ABI's rows");

// a candidate round holds at most this many sites: their windows and the windows' slots are the round's device memory
u64 correct_batch_sites() {
    static const u64 n = getenv("BRISK_CORRECT_BATCH") && atoll(getenv("BRISK_CORRECT_BATCH")) > 0 ? (u64)atoll(getenv("BRISK_CORRECT_BATCH")) : (1ull << 22);
    return n;
}
int check_min_cover(brisk_hip_index* h, u32 min_cover, const char* who, u32* c) {
    if (min_cover > h->P.k) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": min_cover " + std::to_string(min_cover) + " is above k = " + std::to_string(h->P.k));
    *c = min_cover ? min_cover : (u32)h->P.k;
    return BRISK_HIP_OK;
}

// h->corr_tmp: [128 bytes: [0..2] the skipped runs whole / long / short, [4..6] the sites corrected / ambiguous / unresolved, [8] the
// first bad row of a caller's table][block sums behind them, as the pass at hand lays them out]
constexpr size_t kCorrHead = 128;

// The handle's lock is held.  One batch, as split_runs_impl takes it: its weak runs into h->ink_tab, classified and counted into *st
// (a host synchronisation); *n_sites of them are sites, and the block sums that correct_sites_rows needs stay in h->corr_tmp.
int correct_sites_count(brisk_hip_index* h, const uint16_t* d_slots, const u64* d_starts, u64 n_reads, u64 n_slots, u32 solid_min, u32 min_cover, brisk_hip_correct_stats* st,
                        u64* n_runs, u64* n_sites) {
    int rc;
    u64 kept = 0, run_slots = 0, n_short = 0;
    *n_runs = *n_sites = 0;
    if ((rc = split_runs_impl(h, d_slots, d_starts, n_reads, n_slots, solid_min, 1, n_runs, &kept, &run_slots, &n_short, true))) return rc;
    st->n_weak += run_slots;
    st->n_runs += *n_runs;
    if (!*n_runs) return BRISK_HIP_OK;
    const u32 nb = nblocks(*n_runs, 256);
    if ((rc = ensure(h, h->corr_tmp, kCorrHead + ((size_t)nb + 1) * 8))) return rc;
    unsigned long long* d_ctr = (unsigned long long*)h->corr_tmp.p;
    u64* d_bs = (u64*)((char*)h->corr_tmp.p + kCorrHead);
    HIPCHK(h, hipMemsetAsync(d_ctr, 0, kCorrHead, h->stream));
    hipLaunchKernelGGL(k_correct_class, dim3(nb), dim3(256), 0, h->stream, (const IntakeFragment*)h->ink_tab.p, *n_runs, d_starts, (u32)h->P.k, min_cover, d_bs, d_ctr);
    hipLaunchKernelGGL(k_slot_top, dim3(1), dim3(1024), 0, h->stream, d_bs, nb);
    if ((rc = launch_check(h, "k_correct_class / k_slot_top"))) return rc;
    u64 got[4] = {0, 0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(got, d_ctr, 24, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(got + 3, d_bs + nb, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    st->n_skip_whole += got[0];
    st->n_skip_long += got[1];
    st->n_skip_short += got[2];
    st->n_sites += got[3];
    *n_sites = got[3];
    if (got[0] + got[1] + got[2] + got[3] != *n_runs) return fail(h, BRISK_HIP_EHIP, "weak_sites: the classes and the runs disagree");
    return BRISK_HIP_OK;
}
// the sites of the runs that correct_sites_count has just classified, queued on the stream
int correct_sites_rows(brisk_hip_index* h, const u64* d_starts, u64 n_runs, u32 min_cover, CorrectSite* d_out) {
    hipLaunchKernelGGL(k_correct_sites, dim3(nblocks(n_runs, 256)), dim3(256), 0, h->stream, (const IntakeFragment*)h->ink_tab.p, n_runs, d_starts, (u32)h->P.k, min_cover,
                       (const u64*)((char*)h->corr_tmp.p + kCorrHead), d_out);
    return launch_check(h, "k_correct_sites");
}

// a caller's site table against its reads (the read table ascends): EINVAL naming the first bad row
int correct_check_sites(brisk_hip_index* h, const CorrectSite* d_sites, u64 n_sites, const u64* d_starts, u64 n_reads, const char* who) {
    int rc;
    if (!n_sites) return BRISK_HIP_OK;
    if (n_sites > 0x7fffffffull * 256 / 3) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": more rows than one launch covers");
    if ((rc = ensure(h, h->corr_tmp, kCorrHead))) return rc;
    unsigned long long* d_flag = (unsigned long long*)h->corr_tmp.p + 8;
    HIPCHK(h, hipMemsetAsync(d_flag, 0xff, 8, h->stream));
    hipLaunchKernelGGL(k_correct_site_check, dim3(nblocks(n_sites, 256)), dim3(256), 0, h->stream, d_sites, n_sites, d_starts, n_reads, (u32)h->P.k, d_flag);
    if ((rc = launch_check(h, "k_correct_site_check"))) return rc;
    u64 bad = 0;
    HIPCHK(h, hipMemcpyAsync(&bad, d_flag, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bad != ~0ull)
        return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": row " + std::to_string(bad) + " of the site table names a read >= n_reads, has a cover of 0 or above k, or its pos or window lies beyond its read");
    return BRISK_HIP_OK;
}

// The handle's lock is held; the sites are valid.  Their 3 * n_sites candidate windows, substituted, as a packed stream (fragment_gather_impl
// over three rows a site in h->corr_rows, with the candidates' patch).
int correct_windows_impl(brisk_hip_index* h, const u32* d_packed, const u64* d_starts, u64 n_reads, const CorrectSite* d_sites, u64 n_sites, const OutStream& out, const char* who,
                         u64* n_out_nts) {
    int rc;
    if (n_sites) {
        if ((rc = ensure(h, h->corr_rows, 3 * n_sites * 16))) return rc;
        hipLaunchKernelGGL(k_correct_cand_rows, dim3(nblocks(3 * n_sites, 256)), dim3(256), 0, h->stream, d_sites, n_sites, (u32)h->P.k, (IntakeFragment*)h->corr_rows.p);
        if ((rc = launch_check(h, "k_correct_cand_rows"))) return rc;
    }
    return fragment_gather_impl(h, d_packed, d_starts, n_reads, (const IntakeFragment*)h->corr_rows.p, 3 * n_sites, out, false, who, n_out_nts, d_sites);
}

// The handle's lock is held; the sites (n_sites > 0) are valid.  The decisions over the candidates' slots, counted (a host
// synchronisation): cnt[0..2] = corrected / ambiguous / unresolved.  The decisions and the block sums that correct_rows needs stay
// in h->corr_tmp.
int correct_decide_impl(brisk_hip_index* h, const uint16_t* d_cand_slots, const CorrectSite* d_sites, u64 n_sites, const u32* d_packed, const u64* d_starts, u32 solid_min, u64 cnt[3]) {
    int rc;
    const u32 nb = nblocks(n_sites, 256);
    // [head][block sums of the covers, nb + 1][of the corrected sites, nb + 1][a decision a site]
    if ((rc = ensure(h, h->corr_tmp, kCorrHead + 2 * ((size_t)nb + 1) * 8 + n_sites * 4))) return rc;
    unsigned long long* d_ctr = (unsigned long long*)h->corr_tmp.p;
    u64* d_cover = (u64*)((char*)h->corr_tmp.p + kCorrHead);
    u64* d_corr = d_cover + nb + 1;
    u32* d_dec = (u32*)(d_corr + nb + 1);
    HIPCHK(h, hipMemsetAsync(d_ctr, 0, kCorrHead, h->stream));
    hipLaunchKernelGGL(k_correct_cover, dim3(nb), dim3(256), 0, h->stream, d_sites, n_sites, d_cover);
    hipLaunchKernelGGL(k_slot_top, dim3(1), dim3(1024), 0, h->stream, d_cover, nb);
    hipLaunchKernelGGL(k_correct_decide, dim3(nb), dim3(256), 0, h->stream, d_cand_slots, d_sites, n_sites, (const u64*)d_cover, d_packed, d_starts, solid_min, d_dec, d_corr, d_ctr + 4);
    hipLaunchKernelGGL(k_slot_top, dim3(1), dim3(1024), 0, h->stream, d_corr, nb);
    if ((rc = launch_check(h, "k_correct_cover / k_slot_top / k_correct_decide"))) return rc;
    HIPCHK(h, hipMemcpyAsync(cnt, d_ctr + 4, 24, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (cnt[0] + cnt[1] + cnt[2] != n_sites) return fail(h, BRISK_HIP_EHIP, "decide_sites: the decisions and the sites disagree");
    return BRISK_HIP_OK;
}
// the rows of the sites that correct_decide_impl has just found corrected, queued on the stream; r0 is added to their reads
int correct_rows(brisk_hip_index* h, const CorrectSite* d_sites, u64 n_sites, u64 r0, CorrectRow* d_out) {
    const u32 nb = nblocks(n_sites, 256);
    const u64* d_corr = (const u64*)((char*)h->corr_tmp.p + kCorrHead) + nb + 1;
    hipLaunchKernelGGL(k_correct_rows, dim3(nb), dim3(256), 0, h->stream, d_sites, (const u32*)(d_corr + nb + 1), n_sites, d_corr, r0, d_out);
    return launch_check(h, "k_correct_rows");
}

// The handle's lock is held.  brisk_hip_get_kmers_packed's loop over a stream in scratch memory: d_out[n_slots], zeroed here.
int correct_lookups(brisk_hip_index* h, const u32* d_packed, const u64* d_starts, u64 n_reads, uint16_t* d_out, u64 n_slots) {
    int rc;
    HIPCHK(h, hipMemsetAsync(d_out, 0, n_slots * 2, h->stream));
    u64 done = 0;
    for (u64 q0 = 0; q0 < n_reads; q0 += h->max_batch_reads) {
        const u64 nq = std::min<u64>(h->max_batch_reads, n_reads - q0);
        u64 ns = 0;
        if ((rc = count_kmers(h, d_starts + q0, nq, &ns))) return rc;
        if (!ns) continue;
        if (done + ns > n_slots) return fail(h, BRISK_HIP_EHIP, "correct: the candidate stream and its slots disagree");
        if ((rc = kmers_packed_impl(h, d_packed, d_starts + q0, nq, d_out + done, ns))) return rc;
        done += ns;
    }
    if (done != n_slots) return fail(h, BRISK_HIP_EHIP, "correct: the candidate stream and its slots disagree");
    return BRISK_HIP_OK;
}

// One batch of a composed call: d_slots[n_slots] are the slots of the reads of d_starts[0 .. n_reads] (the call's reads from r0 on)
// and h->slot_buf holds their slot bases.  Its sites into h->corr_sites; then, in rounds of at most correct_batch_sites() sites, the
// candidate windows into h->corr_cand, their slots into h->corr_slots (the batch's own slots are no longer needed: the lookups reuse
// the handle's scratch), the decisions, and the correction rows appended to the call's table in h->corr_tab (which grows by copying).
// st->n_corrected: the rows the table holds before the batch.
int correct_batch(brisk_hip_index* h, const u32* d_packed, const uint16_t* d_slots, const u64* d_starts, u64 n_reads, u64 n_slots, u64 r0, u32 solid_min, u32 min_cover,
                  brisk_hip_correct_stats* st) {
    int rc;
    st->n_slots += n_slots;
    if (!n_slots) return BRISK_HIP_OK;
    u64 n_runs = 0, n_sites = 0;
    if ((rc = correct_sites_count(h, d_slots, d_starts, n_reads, n_slots, solid_min, min_cover, st, &n_runs, &n_sites))) return rc;
    if (!n_sites) return BRISK_HIP_OK;
    if ((rc = ensure(h, h->corr_sites, n_sites * 16))) return rc;
    if ((rc = correct_sites_rows(h, d_starts, n_runs, min_cover, (CorrectSite*)h->corr_sites.p))) return rc;
    const u64 k = h->P.k, round = correct_batch_sites();
    for (u64 s0 = 0; s0 < n_sites; s0 += round) {
        const u64 m = std::min<u64>(round, n_sites - s0);
        const CorrectSite* d_sites = (const CorrectSite*)h->corr_sites.p + s0;
        // a window has at most 2 k - 1 nucleotides: [the starts, 3 m + 1][the stream]
        const u64 cap_words = (3 * m * (2 * k - 1) + 15) / 16 + 2;
        const size_t off_packed = ((3 * m + 1) * 8 + 15) / 16 * 16;
        if ((rc = ensure(h, h->corr_cand, off_packed + cap_words * 4))) return rc;
        u64* d_cst = (u64*)h->corr_cand.p;
        u32* d_cpk = (u32*)((char*)h->corr_cand.p + off_packed);
        u64 n_nts = 0;
        if ((rc = correct_windows_impl(h, d_packed, d_starts, n_reads, d_sites, m, {d_cpk, cap_words, d_cst, nullptr}, "correct", &n_nts))) return rc;
        const u64 n_cs = n_nts - 3 * m * (k - 1);  // a window of cover + k - 1 nucleotides has `cover` slots
        if ((rc = ensure(h, h->corr_slots, n_cs * 2))) return rc;
        if ((rc = correct_lookups(h, d_cpk, d_cst, 3 * m, (uint16_t*)h->corr_slots.p, n_cs))) return rc;
        u64 cnt[3] = {0, 0, 0};
        if ((rc = correct_decide_impl(h, (const uint16_t*)h->corr_slots.p, d_sites, m, d_packed, d_starts, solid_min, cnt))) return rc;
        const u64 have = st->n_corrected;
        st->n_corrected += cnt[0];
        st->n_ambiguous += cnt[1];
        st->n_unresolved += cnt[2];
        if (!cnt[0]) continue;
        if (h->corr_tab.bytes < (have + cnt[0]) * 16) {
            DevBuf grown;
            if ((rc = ensure(h, grown, std::max<size_t>((have + cnt[0]) * 16, 2 * h->corr_tab.bytes)))) return rc;
            if (have) HIPCHK(h, hipMemcpyAsync(grown.p, h->corr_tab.p, have * 16, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            if (h->corr_tab.p) HIPCHK(h, hipFree(h->corr_tab.p));
            h->corr_tab = grown;
        }
        if ((rc = correct_rows(h, d_sites, m, r0, (CorrectRow*)h->corr_tab.p + have))) return rc;
    }
    return BRISK_HIP_OK;
}

// the patched copy of words [0, n_words + 2), queued on the stream; the table is valid
int correct_apply_impl(brisk_hip_index* h, const u32* d_packed, const u64* d_starts, const CorrectRow* d_rows, u64 n_rows, u64 n_words, u32* d_out, const char* who) {
    if (n_words + 2 > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, std::string(who) + ": more output words than one launch covers");
    hipLaunchKernelGGL(k_correct_apply, dim3(nblocks(n_words + 2, 256)), dim3(256), 0, h->stream, d_packed, d_starts, d_rows, n_rows, n_words, d_out);
    return launch_check(h, "k_correct_apply");
}

}  // namespace

extern "C" {

// ---- profiles ----
BRISK_API int brisk_hip_read_profile_reads(brisk_hip_index* h, const char* bases, const uint64_t* offsets, uint64_t n_reads, uint32_t solid_min,
                                           brisk_hip_read_profile* out) {
    if (!h || (n_reads && (!bases || !offsets || !out))) return BRISK_HIP_EINVAL;
    if (int wrc = need_whole_index(h, "read_profile_reads")) return wrc;
    if (int orc = check_profile_offsets(h, offsets, n_reads, "read_profile")) return orc;
    if (!n_reads) return BRISK_HIP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    return profile_host_batches(h, bases, offsets, n_reads, solid_min, [&](u64 r0, u64 nr, const ReadProfile* d_prof) -> int {
        HIPCHK(h, hipMemcpyAsync(out + r0, d_prof, nr * sizeof(ReadProfile), hipMemcpyDeviceToHost, h->stream));
        return BRISK_HIP_OK;
    });
}

BRISK_API int brisk_hip_read_profile_packed(brisk_hip_index* h, const uint32_t* d_packed, const uint64_t* d_starts, uint64_t n_reads, uint32_t solid_min,
                                            brisk_hip_read_profile* d_out) {
    if (!h || (n_reads && (!d_packed || !d_starts || !d_out))) return BRISK_HIP_EINVAL;
    if (int wrc = need_whole_index(h, "read_profile_packed")) return wrc;
    if (!n_reads) return BRISK_HIP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    // (the records are the output: nothing follows a batch)
    if (int rc = profile_packed_batches(h, d_packed, d_starts, n_reads, solid_min, [&](u64 r0) { return (ReadProfile*)d_out + r0; }, [](u64, u64, const ReadProfile*) { return BRISK_HIP_OK; })) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return check_device_flags(h);
}

// ---- select, extract, trim ----

BRISK_API int brisk_hip_select_intervals(brisk_hip_index* h, const brisk_hip_read_profile* d_profiles, uint64_t n_reads, const brisk_hip_select_rule* rule,
                                         brisk_hip_read_interval* d_intervals) {
    if (!h) return BRISK_HIP_EINVAL;
    if (int rrc = check_rule(h, rule, "select_intervals")) return rrc;
    if (n_reads && (!d_profiles || !d_intervals)) return fail(h, BRISK_HIP_EINVAL, "select_intervals: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int rc = select_impl(h, (const ReadProfile*)d_profiles, n_reads, rule, (ReadInterval*)d_intervals)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_extract_packed(brisk_hip_index* h, const uint32_t* d_packed, const uint64_t* d_starts, uint64_t n_reads, const brisk_hip_read_interval* d_intervals,
                                       uint32_t* d_out_packed, uint64_t out_cap_words, uint64_t* d_out_starts, uint64_t* d_out_index, uint64_t* n_out_reads,
                                       uint64_t* n_out_nts) {
    if (!h) return BRISK_HIP_EINVAL;
    if (!n_out_reads || !n_out_nts || !d_out_packed || !d_out_starts || (n_reads && (!d_packed || !d_starts || !d_intervals))) return fail(h, BRISK_HIP_EINVAL, "extract_packed: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    return extract_impl(h, d_packed, d_starts, n_reads, (const ReadInterval*)d_intervals, {d_out_packed, out_cap_words, d_out_starts, d_out_index}, n_out_reads, n_out_nts);
}

BRISK_API int brisk_hip_trim_packed(brisk_hip_index* h, const uint32_t* d_packed, const uint64_t* d_starts, uint64_t n_reads, uint32_t solid_min, const brisk_hip_select_rule* rule,
                                    uint32_t* d_out_packed, uint64_t out_cap_words, uint64_t* d_out_starts, uint64_t* d_out_index, uint64_t* n_out_reads, uint64_t* n_out_nts) {
    if (!h) return BRISK_HIP_EINVAL;
    if (int wrc = need_whole_index(h, "trim_packed")) return wrc;
    if (int rrc = check_rule(h, rule, "trim_packed")) return rrc;
    if (!n_out_reads || !n_out_nts || !d_out_packed || !d_out_starts || (n_reads && (!d_packed || !d_starts))) return fail(h, BRISK_HIP_EINVAL, "trim_packed: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    int rc;
    if (n_reads) {
        if ((rc = ensure(h, h->ext_iv, n_reads * sizeof(ReadInterval)))) return rc;
        if ((rc = profile_select(h, d_packed, d_starts, n_reads, solid_min, rule, (ReadInterval*)h->ext_iv.p, nullptr))) return rc;
    }
    return extract_impl(h, d_packed, d_starts, n_reads, (const ReadInterval*)h->ext_iv.p, {d_out_packed, out_cap_words, d_out_starts, d_out_index}, n_out_reads, n_out_nts);
}

BRISK_API int brisk_hip_trim_reads(brisk_hip_index* h, const char* bases, const uint64_t* offsets, uint64_t n_reads, uint32_t solid_min, const brisk_hip_select_rule* rule,
                                   brisk_hip_read_interval* out) {
    if (!h) return BRISK_HIP_EINVAL;
    if (int wrc = need_whole_index(h, "trim_reads")) return wrc;
    if (int rrc = check_rule(h, rule, "trim_reads")) return rrc;
    if (n_reads && (!bases || !offsets || !out)) return fail(h, BRISK_HIP_EINVAL, "trim_reads: null pointer");
    if (int orc = check_profile_offsets(h, offsets, n_reads, "trim_reads")) return orc;
    if (!n_reads) return BRISK_HIP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    return profile_host_batches(h, bases, offsets, n_reads, solid_min, [&](u64 r0, u64 nr, const ReadProfile* d_prof) -> int {
        int rc;
        if ((rc = ensure(h, h->ext_iv, nr * sizeof(ReadInterval)))) return rc;
        if ((rc = select_impl(h, d_prof, nr, rule, (ReadInterval*)h->ext_iv.p))) return rc;
        HIPCHK(h, hipMemcpyAsync(out + r0, h->ext_iv.p, nr * sizeof(ReadInterval), hipMemcpyDeviceToHost, h->stream));
        return BRISK_HIP_OK;
    });
}

// ---- intake ----
BRISK_API int brisk_hip_intake_ascii(brisk_hip_index* h, const char* d_bases, const char* d_quals, const uint64_t* d_offsets, uint64_t n_reads, const brisk_hip_intake_rule* rule,
                                     uint32_t* d_out_packed, uint64_t out_cap_words, uint64_t* d_out_starts, brisk_hip_fragment* d_out_frags, uint64_t frag_cap,
                                     brisk_hip_intake_stats* stats) {
    if (!h) return BRISK_HIP_EINVAL;
    u32 min_len = 0, thr = 0;
    if (int rrc = check_intake_rule(h, rule, d_quals != nullptr, "intake_ascii", &min_len, &thr)) return rrc;
    if (!stats || !d_out_starts || (n_reads && (!d_bases || !d_offsets))) return fail(h, BRISK_HIP_EINVAL, "intake_ascii: null pointer");
    if (!d_out_packed && out_cap_words) return fail(h, BRISK_HIP_EINVAL, "intake_ascii: out_cap_words without d_out_packed");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    return intake_impl(h, (const uint8_t*)d_bases, (const uint8_t*)d_quals, d_offsets, n_reads, min_len, thr, d_out_packed, out_cap_words, d_out_starts, (IntakeFragment*)d_out_frags,
                       frag_cap, stats);
}

BRISK_API int brisk_hip_intake_reads(brisk_hip_index* h, const char* bases, const char* quals, const uint64_t* offsets, uint64_t n_reads, const brisk_hip_intake_rule* rule,
                                     brisk_hip_fragment* out_frags, uint64_t frag_cap, brisk_hip_intake_stats* stats) {
    if (!h) return BRISK_HIP_EINVAL;
    u32 min_len = 0, thr = 0;
    if (int rrc = check_intake_rule(h, rule, quals != nullptr, "intake_reads", &min_len, &thr)) return rrc;
    if (!stats || (frag_cap && !out_frags) || (n_reads && (!bases || !offsets))) return fail(h, BRISK_HIP_EINVAL, "intake_reads: null pointer");
    if (int orc = check_raw_reads(h, offsets, n_reads, "intake_reads")) return orc;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    memset(stats, 0, sizeof(*stats));
    int rc = for_each_raw_piece(h, bases, thr ? quals : nullptr, offsets, n_reads, [&](u64 r0, u64 nr, const uint8_t* d_b, const uint8_t* d_q, const u64* d_offs) -> int {
        brisk_hip_intake_stats st;
        if (int rc2 = intake_impl(h, d_b, d_q, d_offs, nr, min_len, thr, nullptr, 0, nullptr, nullptr, ~0ull, &st)) return rc2;
        const u64 at = stats->n_fragments;
        if (st.n_fragments && at + st.n_fragments <= frag_cap) {  // (past the caller's room the pieces are still counted: the stats are whole)
            HIPCHK(h, hipMemcpyAsync(out_frags + at, h->ink_tab.p, st.n_fragments * 16, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            for (u64 j = 0; j < st.n_fragments; j++) out_frags[at + j].read += r0;  // the device counted the piece's reads
        }
        add_counters(stats, st);
        return BRISK_HIP_OK;
    });
    if (rc) return rc;
    if (stats->n_fragments > frag_cap) return fail(h, BRISK_HIP_ECAPACITY, "intake_reads: " + std::to_string(stats->n_fragments) + " fragments, frag_cap is " + std::to_string(frag_cap));
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_insert_raw_reads(brisk_hip_index* h, const char* bases, const char* quals, const uint64_t* offsets, uint64_t n_reads, const brisk_hip_intake_rule* rule,
                                         brisk_hip_intake_stats* stats) {
    if (!h || (n_reads && (!bases || !offsets))) return BRISK_HIP_EINVAL;
    if (h->P.n_owners > 1) return fail(h, BRISK_HIP_EINVAL, "insert_reads on a sharded index: use scan/route/insert_records");
    if (h->entry_ids) return fail(h, BRISK_HIP_EINVAL, "bulk count on an entry-id index");
    u32 min_len = 0, thr = 0;
    if (int rrc = check_intake_rule(h, rule, quals != nullptr, "insert_raw_reads", &min_len, &thr)) return rrc;
    if (int orc = check_raw_reads(h, offsets, n_reads, "insert_raw_reads")) return orc;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    brisk_hip_intake_stats sum = {};
    if (stats) *stats = sum;
    int rc = for_each_raw_piece(h, bases, thr ? quals : nullptr, offsets, n_reads, [&](u64 r0, u64 nr, const uint8_t* d_b, const uint8_t* d_q, const u64* d_offs) -> int {
        // the piece's packed stream and its starts: what always suffices (include/brisk_hip.h)
        const u64 nb = offsets[r0 + nr] - offsets[r0], cap_words = (nb + 15) / 16 + 2, cap_frag = nb / min_len, words_room = (cap_words + 1) & ~1ull;
        if (int rc2 = ensure(h, h->ink_packed, words_room * 4 + (cap_frag + 1) * 8)) return rc2;
        u32* d_packed = (u32*)h->ink_packed.p;
        u64* d_starts = (u64*)(d_packed + words_room);
        brisk_hip_intake_stats st;
        if (int rc2 = intake_impl(h, d_b, d_q, d_offs, nr, min_len, thr, d_packed, cap_words, d_starts, nullptr, cap_frag, &st)) return rc2;
        add_counters(&sum, st);
        // the scan of this stream is queued before insert_packed_impl returns (a deferred insert keeps records, not the stream), and the
        // next piece's writes follow it on the handle's stream: the scratch is free for them
        return insert_packed_impl(h, d_packed, d_starts, st.n_fragments);
    });
    if (stats) *stats = sum;
    return rc;
}

// ---- paired-end reads ----
BRISK_API int brisk_hip_fragment_intervals(brisk_hip_index* h, const brisk_hip_fragment* d_frags, uint64_t n_frags, uint64_t n_reads, brisk_hip_read_interval* d_intervals) {
    if (!h) return BRISK_HIP_EINVAL;
    if ((n_frags && !d_frags) || (n_reads && !d_intervals)) return fail(h, BRISK_HIP_EINVAL, "fragment_intervals: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int rc = fragment_intervals_impl(h, (const IntakeFragment*)d_frags, n_frags, n_reads, (ReadInterval*)d_intervals)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_pair_intervals(brisk_hip_index* h, const brisk_hip_read_interval* d_each, const brisk_hip_read_interval* d_whole, uint64_t n_reads, uint32_t pair_mode,
                                       brisk_hip_read_interval* d_out) {
    if (!h) return BRISK_HIP_EINVAL;
    if (int crc = check_pairs(h, n_reads, pair_mode, "pair_intervals")) return crc;
    if (pair_mode == BRISK_HIP_PAIR_ANY && !d_whole) return fail(h, BRISK_HIP_EINVAL, "pair_intervals: BRISK_HIP_PAIR_ANY needs d_whole");
    if (n_reads && (!d_each || !d_out)) return fail(h, BRISK_HIP_EINVAL, "pair_intervals: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int rc = pair_intervals_impl(h, (const ReadInterval*)d_each, (const ReadInterval*)d_whole, n_reads, pair_mode, (ReadInterval*)d_out)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_compose_intervals(brisk_hip_index* h, const brisk_hip_read_interval* d_outer, uint64_t n_reads, const brisk_hip_read_interval* d_inner, const uint64_t* d_index,
                                          uint64_t n_kept, brisk_hip_read_interval* d_out) {
    if (!h) return BRISK_HIP_EINVAL;
    if ((n_reads && !d_out) || (n_kept && (!d_outer || !d_inner || !d_index))) return fail(h, BRISK_HIP_EINVAL, "compose_intervals: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int rc = compose_impl(h, (const ReadInterval*)d_outer, n_reads, (const ReadInterval*)d_inner, d_index, n_kept, (ReadInterval*)d_out)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_extract_pairs_packed(brisk_hip_index* h, const uint32_t* d_packed, const uint64_t* d_starts, uint64_t n_reads, const brisk_hip_read_interval* d_intervals,
                                             uint32_t* d_pairs_packed, uint64_t pairs_cap_words, uint64_t* d_pairs_starts, uint64_t* d_pairs_index, uint32_t* d_singles_packed,
                                             uint64_t singles_cap_words, uint64_t* d_singles_starts, uint64_t* d_singles_index, brisk_hip_pair_counts* counts) {
    if (!h) return BRISK_HIP_EINVAL;
    const OutStream P = {d_pairs_packed, pairs_cap_words, d_pairs_starts, d_pairs_index}, S = {d_singles_packed, singles_cap_words, d_singles_starts, d_singles_index};
    if (int orc = check_pair_outs(h, P, S, counts, "extract_pairs_packed")) return orc;
    if (n_reads && (!d_packed || !d_starts || !d_intervals)) return fail(h, BRISK_HIP_EINVAL, "extract_pairs_packed: null pointer");
    if (int crc = check_pairs(h, n_reads, BRISK_HIP_PAIR_EACH, "extract_pairs_packed")) return crc;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    return extract_pairs_impl(h, d_packed, d_starts, n_reads, (const ReadInterval*)d_intervals, P, S, counts);
}

BRISK_API int brisk_hip_trim_pairs_packed(brisk_hip_index* h, const uint32_t* d_packed, const uint64_t* d_starts, uint64_t n_reads, uint32_t solid_min, const brisk_hip_select_rule* rule,
                                          uint32_t pair_mode, uint32_t* d_pairs_packed, uint64_t pairs_cap_words, uint64_t* d_pairs_starts, uint64_t* d_pairs_index,
                                          uint32_t* d_singles_packed, uint64_t singles_cap_words, uint64_t* d_singles_starts, uint64_t* d_singles_index, brisk_hip_pair_counts* counts) {
    if (!h) return BRISK_HIP_EINVAL;
    if (int wrc = need_whole_index(h, "trim_pairs_packed")) return wrc;
    if (int rrc = check_rule(h, rule, "trim_pairs_packed")) return rrc;
    if (int crc = check_pairs(h, n_reads, pair_mode, "trim_pairs_packed")) return crc;
    const OutStream P = {d_pairs_packed, pairs_cap_words, d_pairs_starts, d_pairs_index}, S = {d_singles_packed, singles_cap_words, d_singles_starts, d_singles_index};
    if (int orc = check_pair_outs(h, P, S, counts, "trim_pairs_packed")) return orc;
    if (n_reads && (!d_packed || !d_starts)) return fail(h, BRISK_HIP_EINVAL, "trim_pairs_packed: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    int rc;
    const bool any = pair_mode == BRISK_HIP_PAIR_ANY;
    if (n_reads) {
        if ((rc = ensure(h, h->ext_iv, n_reads * sizeof(ReadInterval)))) return rc;
        if (any && (rc = ensure(h, h->pair_iv, n_reads * sizeof(ReadInterval)))) return rc;
        ReadInterval* d_each = (ReadInterval*)h->ext_iv.p;
        ReadInterval* d_whole = any ? (ReadInterval*)h->pair_iv.p : nullptr;
        if ((rc = profile_select(h, d_packed, d_starts, n_reads, solid_min, rule, d_each, d_whole))) return rc;
        if ((rc = pair_intervals_impl(h, d_each, d_whole, n_reads, pair_mode, d_each))) return rc;
    }
    return extract_pairs_impl(h, d_packed, d_starts, n_reads, (const ReadInterval*)h->ext_iv.p, P, S, counts);
}

BRISK_API int brisk_hip_trim_pairs_reads(brisk_hip_index* h, const char* bases, const uint64_t* offsets, uint64_t n_reads, uint32_t solid_min, const brisk_hip_select_rule* rule,
                                         uint32_t pair_mode, brisk_hip_read_interval* out, brisk_hip_pair_counts* counts) {
    if (!h) return BRISK_HIP_EINVAL;
    if (int wrc = need_whole_index(h, "trim_pairs_reads")) return wrc;
    if (int rrc = check_rule(h, rule, "trim_pairs_reads")) return rrc;
    if (int crc = check_pairs(h, n_reads, pair_mode, "trim_pairs_reads")) return crc;
    if (!counts || (n_reads && (!bases || !offsets || !out))) return fail(h, BRISK_HIP_EINVAL, "trim_pairs_reads: null pointer");
    if (int orc = check_profile_offsets(h, offsets, n_reads, "trim_pairs_reads")) return orc;
    memset(counts, 0, sizeof(*counts));
    if (!n_reads) return BRISK_HIP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    int rc;
    // the whole call's intervals stay on the device until the pair decision: a batch may end between two mates
    const bool any = pair_mode == BRISK_HIP_PAIR_ANY;
    if ((rc = ensure(h, h->ext_iv, n_reads * sizeof(ReadInterval)))) return rc;
    if (any && (rc = ensure(h, h->pair_iv, n_reads * sizeof(ReadInterval)))) return rc;
    ReadInterval* d_each = (ReadInterval*)h->ext_iv.p;
    ReadInterval* d_whole = any ? (ReadInterval*)h->pair_iv.p : nullptr;
    rc = profile_host_batches(h, bases, offsets, n_reads, solid_min,
                              [&](u64 r0, u64 nr, const ReadProfile* d_prof) { return select_batch(h, d_prof, nr, rule, d_each + r0, any ? d_whole + r0 : nullptr); });
    if (rc) return rc;
    if ((rc = pair_intervals_impl(h, d_each, d_whole, n_reads, pair_mode, d_each))) return rc;
    const ReadInterval *iv_p, *iv_s;
    if ((rc = pair_split_impl(h, d_each, n_reads, nullptr, counts, &iv_p, &iv_s))) return rc;
    HIPCHK(h, hipMemcpyAsync(out, d_each, n_reads * sizeof(ReadInterval), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_clean_pairs_ascii(brisk_hip_index* h, const char* d_bases, const char* d_quals, const uint64_t* d_offsets, uint64_t n_reads, const brisk_hip_intake_rule* intake,
                                          const brisk_hip_select_rule* select, uint32_t solid_min, uint32_t pair_mode, uint32_t* d_pairs_packed, uint64_t pairs_cap_words,
                                          uint64_t* d_pairs_starts, uint64_t* d_pairs_index, uint32_t* d_singles_packed, uint64_t singles_cap_words, uint64_t* d_singles_starts,
                                          uint64_t* d_singles_index, brisk_hip_read_interval* d_out_intervals, brisk_hip_pair_counts* counts, brisk_hip_intake_stats* stats) {
    if (!h) return BRISK_HIP_EINVAL;
    u32 min_len = 0, thr = 0;
    if (int crc = check_clean_pairs(h, intake, d_quals != nullptr, select, n_reads, pair_mode, "clean_pairs_ascii", &min_len, &thr)) return crc;
    const OutStream P = {d_pairs_packed, pairs_cap_words, d_pairs_starts, d_pairs_index}, S = {d_singles_packed, singles_cap_words, d_singles_starts, d_singles_index};
    if (int orc = check_pair_outs(h, P, S, counts, "clean_pairs_ascii")) return orc;
    if (!stats || (n_reads && (!d_bases || !d_offsets))) return fail(h, BRISK_HIP_EINVAL, "clean_pairs_ascii: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (select)
        if (int frc = enter(h)) return frc;
    int rc;
    CleanedPairs c;
    if ((rc = clean_pairs_core(h, (const uint8_t*)d_bases, (const uint8_t*)d_quals, d_offsets, n_reads, min_len, thr, select, solid_min, pair_mode, stats, &c))) return rc;
    if ((rc = extract_pairs_impl(h, c.raw, c.raw_starts, n_reads, c.intervals, P, S, counts))) return rc;
    if (d_out_intervals && n_reads) {
        HIPCHK(h, hipMemcpyAsync(d_out_intervals, c.intervals, n_reads * sizeof(ReadInterval), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_clean_pairs_reads(brisk_hip_index* h, const char* bases, const char* quals, const uint64_t* offsets, uint64_t n_reads, const brisk_hip_intake_rule* intake,
                                          const brisk_hip_select_rule* select, uint32_t solid_min, uint32_t pair_mode, brisk_hip_read_interval* out, brisk_hip_pair_counts* counts,
                                          brisk_hip_intake_stats* stats) {
    if (!h) return BRISK_HIP_EINVAL;
    u32 min_len = 0, thr = 0;
    if (int crc = check_clean_pairs(h, intake, quals != nullptr, select, n_reads, pair_mode, "clean_pairs_reads", &min_len, &thr)) return crc;
    if (!stats || !counts || (n_reads && (!bases || !offsets || !out))) return fail(h, BRISK_HIP_EINVAL, "clean_pairs_reads: null pointer");
    if (int orc = check_raw_reads(h, offsets, n_reads, "clean_pairs_reads")) return orc;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    memset(stats, 0, sizeof(*stats));
    memset(counts, 0, sizeof(*counts));
    if (select)
        if (int frc = enter(h)) return frc;
    return for_each_raw_piece(h, bases, thr ? quals : nullptr, offsets, n_reads, [&](u64 r0, u64 nr, const uint8_t* d_b, const uint8_t* d_q, const u64* d_offs) -> int {
        int rc2;
        brisk_hip_intake_stats st;
        brisk_hip_pair_counts pc;
        CleanedPairs c;
        const ReadInterval *iv_p, *iv_s;
        if ((rc2 = clean_pairs_core(h, d_b, d_q, d_offs, nr, min_len, thr, select, solid_min, pair_mode, &st, &c))) return rc2;
        if ((rc2 = pair_split_impl(h, c.intervals, nr, nullptr, &pc, &iv_p, &iv_s))) return rc2;
        HIPCHK(h, hipMemcpyAsync(out + r0, c.intervals, nr * sizeof(ReadInterval), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        add_counters(stats, st);
        add_counters(counts, pc);
        return BRISK_HIP_OK;
    }, 2);
}

// ---- read splitting ----
BRISK_API int brisk_hip_solid_runs(brisk_hip_index* h, const uint16_t* d_slots, const uint64_t* d_starts, uint64_t n_reads, uint32_t solid_min, uint32_t min_len,
                                   brisk_hip_fragment* d_out_frags, uint64_t frag_cap, brisk_hip_split_stats* stats) {
    if (!h) return BRISK_HIP_EINVAL;
    if (!stats || (n_reads && !d_starts) || (frag_cap && !d_out_frags)) return fail(h, BRISK_HIP_EINVAL, "solid_runs: null pointer");
    memset(stats, 0, sizeof(*stats));
    stats->n_reads = n_reads;
    if (!n_reads) return BRISK_HIP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    int rc;
    u64 ns = 0, nf = 0, run_slots = 0;
    if ((rc = split_check_table(h, d_starts, n_reads, "solid_runs", true, &stats->n_nts_in))) return rc;
    if ((rc = count_kmers(h, d_starts, n_reads, &ns))) return rc;
    stats->n_slots = ns;
    if (!ns) return BRISK_HIP_OK;
    if (!d_slots) return fail(h, BRISK_HIP_EINVAL, "solid_runs: null pointer");
    if ((rc = slot_bases(h, d_starts, n_reads))) return rc;
    if ((rc = split_runs_impl(h, d_slots, d_starts, n_reads, ns, solid_min, split_min_slots(h, min_len), &nf, &stats->n_reads_kept, &run_slots, &stats->n_short))) return rc;
    stats->n_fragments = nf;
    stats->n_solid = run_slots + stats->n_short;
    stats->n_nts_out = run_slots + nf * (h->P.k - 1);
    if (frag_cap < nf) return fail(h, BRISK_HIP_ECAPACITY, "solid_runs: " + std::to_string(nf) + " fragments, frag_cap is " + std::to_string(frag_cap));
    if (!nf) return BRISK_HIP_OK;
    if ((rc = split_rows(h, nf, 0, (IntakeFragment*)d_out_frags))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_extract_fragments_packed(brisk_hip_index* h, const uint32_t* d_packed, const uint64_t* d_starts, uint64_t n_reads, const brisk_hip_fragment* d_frags,
                                                 uint64_t n_frags, uint32_t* d_out_packed, uint64_t out_cap_words, uint64_t* d_out_starts, uint64_t* n_out_nts) {
    if (!h) return BRISK_HIP_EINVAL;
    if (!n_out_nts || !d_out_packed || !d_out_starts || (n_reads && (!d_packed || !d_starts)) || (n_frags && !d_frags)) return fail(h, BRISK_HIP_EINVAL, "extract_fragments_packed: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    return fragment_gather_impl(h, d_packed, d_starts, n_reads, (const IntakeFragment*)d_frags, n_frags, {d_out_packed, out_cap_words, d_out_starts, nullptr}, true,
                                "extract_fragments_packed", n_out_nts);
}

BRISK_API int brisk_hip_split_packed(brisk_hip_index* h, const uint32_t* d_packed, const uint64_t* d_starts, uint64_t n_reads, uint32_t solid_min, uint32_t min_len,
                                     uint32_t* d_out_packed, uint64_t out_cap_words, uint64_t* d_out_starts, brisk_hip_fragment* d_out_frags, uint64_t frag_cap,
                                     brisk_hip_split_stats* stats) {
    if (!h) return BRISK_HIP_EINVAL;
    if (int wrc = need_whole_index(h, "split_packed")) return wrc;
    if (!stats || !d_out_starts || (n_reads && (!d_packed || !d_starts))) return fail(h, BRISK_HIP_EINVAL, "split_packed: null pointer");
    if (!d_out_packed && out_cap_words) return fail(h, BRISK_HIP_EINVAL, "split_packed: out_cap_words without d_out_packed");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    int rc;
    memset(stats, 0, sizeof(*stats));
    stats->n_reads = n_reads;
    if (n_reads) {
        if ((rc = split_check_table(h, d_starts, n_reads, "split_packed", true, &stats->n_nts_in))) return rc;
        // a sibling of profile_packed_batches: a batch's slots into kout_tmp, and its runs instead of its records
        const u64 batch = profile_batch_limit(h);
        const u32 min_slots = split_min_slots(h, min_len);
        for (u64 r0 = 0; r0 < n_reads; r0 += batch) {
            const u64 nb = std::min<u64>(batch, n_reads - r0);
            u64 ns = 0;
            if ((rc = count_kmers(h, d_starts + r0, nb, &ns))) return rc;
            if (ns) {
                if ((rc = ensure(h, h->kout_tmp, ns * 2))) return rc;
                HIPCHK(h, hipMemsetAsync(h->kout_tmp.p, 0, ns * 2, h->stream));
                if ((rc = kmers_packed_impl(h, d_packed, d_starts + r0, nb, (uint16_t*)h->kout_tmp.p, ns))) return rc;
            }
            if ((rc = split_batch(h, (const uint16_t*)h->kout_tmp.p, d_starts + r0, nb, ns, r0, solid_min, min_slots, stats))) return rc;
        }
        if ((rc = check_device_flags(h))) return rc;
    }
    const u64 nf = stats->n_fragments, need_words = (stats->n_nts_out + 15) / 16 + 2;
    if (frag_cap < nf) return fail(h, BRISK_HIP_ECAPACITY, "split_packed: " + std::to_string(nf) + " fragments, frag_cap is " + std::to_string(frag_cap));
    if (d_out_packed && out_cap_words < need_words)
        return fail(h, BRISK_HIP_ECAPACITY, "split_packed: " + std::to_string(stats->n_nts_out) + " nucleotides need " + std::to_string(need_words) + " words, out_cap_words is " + std::to_string(out_cap_words));
    u64 n_nts = 0;
    if ((rc = fragment_gather_impl(h, d_packed, d_starts, n_reads, (const IntakeFragment*)h->split_tab.p, nf, {d_out_packed, out_cap_words, d_out_starts, nullptr}, false, "split_packed", &n_nts))) return rc;
    if (n_nts != stats->n_nts_out) return fail(h, BRISK_HIP_EHIP, "split_packed: the stream and the counters disagree");
    if (d_out_frags && nf) {
        HIPCHK(h, hipMemcpyAsync(d_out_frags, h->split_tab.p, nf * 16, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_split_reads(brisk_hip_index* h, const char* bases, const uint64_t* offsets, uint64_t n_reads, uint32_t solid_min, uint32_t min_len,
                                    brisk_hip_fragment* out_frags, uint64_t frag_cap, brisk_hip_split_stats* stats) {
    if (!h) return BRISK_HIP_EINVAL;
    if (int wrc = need_whole_index(h, "split_reads")) return wrc;
    if (!stats || (frag_cap && !out_frags) || (n_reads && (!bases || !offsets))) return fail(h, BRISK_HIP_EINVAL, "split_reads: null pointer");
    for (u64 r = 0; r < n_reads; r++) {
        if (offsets[r + 1] < offsets[r]) return fail(h, BRISK_HIP_EINVAL, "read offsets do not ascend (offsets[i + 1] < offsets[i])");
        if (offsets[r + 1] - offsets[r] > 0xffffffffull) return fail(h, BRISK_HIP_EINVAL, "split_reads: a read of 2^32 nucleotides or more does not fit the fragment record");
    }
    memset(stats, 0, sizeof(*stats));
    stats->n_reads = n_reads;
    if (!n_reads) return BRISK_HIP_OK;
    stats->n_nts_in = offsets[n_reads] - offsets[0];
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    const u32 min_slots = split_min_slots(h, min_len);
    // profile_batch has left the batch's slots in kout_tmp and their bases in slot_buf: the runs are taken from them
    int rc = profile_host_batches(h, bases, offsets, n_reads, solid_min, [&](u64 r0, u64 nr, const ReadProfile*) -> int {
        return split_batch(h, (const uint16_t*)h->kout_tmp.p, (const u64*)h->starts_tmp.p, nr, host_slots(offsets, r0, r0 + nr, h->P.k), r0, solid_min, min_slots, stats);
    });
    if (rc) return rc;
    const u64 nf = stats->n_fragments;
    if (frag_cap < nf) return fail(h, BRISK_HIP_ECAPACITY, "split_reads: " + std::to_string(nf) + " fragments, frag_cap is " + std::to_string(frag_cap));
    if (nf) {
        HIPCHK(h, hipMemcpyAsync(out_frags, h->split_tab.p, nf * 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return BRISK_HIP_OK;
}

// ---- spectral read correction ----
BRISK_API int brisk_hip_weak_sites(brisk_hip_index* h, const uint16_t* d_slots, const uint64_t* d_starts, uint64_t n_reads, uint32_t solid_min, uint32_t min_cover,
                                   brisk_hip_site* d_out_sites, uint64_t site_cap, brisk_hip_correct_stats* stats) {
    if (!h) return BRISK_HIP_EINVAL;
    if (!stats || (n_reads && !d_starts) || (site_cap && !d_out_sites)) return fail(h, BRISK_HIP_EINVAL, "weak_sites: null pointer");
    u32 c = 0;
    if (int crc = check_min_cover(h, min_cover, "weak_sites", &c)) return crc;
    memset(stats, 0, sizeof(*stats));
    stats->n_reads = n_reads;
    if (!n_reads) return BRISK_HIP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    int rc;
    u64 ns = 0, n_nts = 0, n_runs = 0, n_sites = 0;
    if ((rc = split_check_table(h, d_starts, n_reads, "weak_sites", true, &n_nts))) return rc;
    if ((rc = count_kmers(h, d_starts, n_reads, &ns))) return rc;
    stats->n_slots = ns;
    if (!ns) return BRISK_HIP_OK;
    if (!d_slots) return fail(h, BRISK_HIP_EINVAL, "weak_sites: null pointer");
    if ((rc = slot_bases(h, d_starts, n_reads))) return rc;
    if ((rc = correct_sites_count(h, d_slots, d_starts, n_reads, ns, solid_min, c, stats, &n_runs, &n_sites))) return rc;
    if (site_cap < n_sites) return fail(h, BRISK_HIP_ECAPACITY, "weak_sites: " + std::to_string(n_sites) + " sites, site_cap is " + std::to_string(site_cap));
    if (!n_sites) return BRISK_HIP_OK;
    if ((rc = correct_sites_rows(h, d_starts, n_runs, c, (CorrectSite*)d_out_sites))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_candidate_windows(brisk_hip_index* h, const uint32_t* d_packed, const uint64_t* d_starts, uint64_t n_reads, const brisk_hip_site* d_sites, uint64_t n_sites,
                                          uint32_t* d_out_packed, uint64_t out_cap_words, uint64_t* d_out_starts, uint64_t* n_out_nts) {
    if (!h) return BRISK_HIP_EINVAL;
    if (!n_out_nts || !d_out_packed || !d_out_starts || (n_reads && (!d_packed || !d_starts)) || (n_sites && !d_sites)) return fail(h, BRISK_HIP_EINVAL, "candidate_windows: null pointer");
    *n_out_nts = 0;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    int rc;
    u64 unused = 0;
    if (n_reads && (rc = split_check_table(h, d_starts, n_reads, "candidate_windows", false, &unused))) return rc;
    if ((rc = correct_check_sites(h, (const CorrectSite*)d_sites, n_sites, d_starts, n_reads, "candidate_windows"))) return rc;
    return correct_windows_impl(h, d_packed, d_starts, n_reads, (const CorrectSite*)d_sites, n_sites, {d_out_packed, out_cap_words, d_out_starts, nullptr}, "candidate_windows", n_out_nts);
}

BRISK_API int brisk_hip_decide_sites(brisk_hip_index* h, const uint16_t* d_cand_slots, const brisk_hip_site* d_sites, uint64_t n_sites, const uint32_t* d_packed,
                                     const uint64_t* d_starts, uint64_t n_reads, uint32_t solid_min, brisk_hip_correction* d_out_corrections, uint64_t corr_cap,
                                     brisk_hip_correct_stats* stats) {
    if (!h) return BRISK_HIP_EINVAL;
    if (!stats || (n_reads && (!d_packed || !d_starts)) || (n_sites && (!d_sites || !d_cand_slots)) || (corr_cap && !d_out_corrections))
        return fail(h, BRISK_HIP_EINVAL, "decide_sites: null pointer");
    memset(stats, 0, sizeof(*stats));
    if (!n_sites) return BRISK_HIP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    int rc;
    u64 unused = 0, cnt[3] = {0, 0, 0};
    if (n_reads && (rc = split_check_table(h, d_starts, n_reads, "decide_sites", false, &unused))) return rc;
    if ((rc = correct_check_sites(h, (const CorrectSite*)d_sites, n_sites, d_starts, n_reads, "decide_sites"))) return rc;
    if ((rc = correct_decide_impl(h, d_cand_slots, (const CorrectSite*)d_sites, n_sites, d_packed, d_starts, solid_min, cnt))) return rc;
    stats->n_sites = n_sites;
    stats->n_corrected = cnt[0];
    stats->n_ambiguous = cnt[1];
    stats->n_unresolved = cnt[2];
    if (corr_cap < cnt[0]) return fail(h, BRISK_HIP_ECAPACITY, "decide_sites: " + std::to_string(cnt[0]) + " corrections, corr_cap is " + std::to_string(corr_cap));
    if (!cnt[0]) return BRISK_HIP_OK;
    if ((rc = correct_rows(h, (const CorrectSite*)d_sites, n_sites, 0, (CorrectRow*)d_out_corrections))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_apply_corrections(brisk_hip_index* h, const uint32_t* d_packed, const uint64_t* d_starts, uint64_t n_reads, const brisk_hip_correction* d_corr,
                                          uint64_t n_corr, uint32_t* d_out_packed, uint64_t out_cap_words) {
    if (!h) return BRISK_HIP_EINVAL;
    if (!d_out_packed || (n_reads && (!d_packed || !d_starts)) || (n_corr && !d_corr)) return fail(h, BRISK_HIP_EINVAL, "apply_corrections: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    int rc;
    u64 unused = 0, last = 0;
    if (n_reads) {
        if ((rc = split_check_table(h, d_starts, n_reads, "apply_corrections", false, &unused))) return rc;
        HIPCHK(h, hipMemcpyAsync(&last, d_starts + n_reads, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (n_corr) {
        if (n_corr > 0x7fffffffull * 256) return fail(h, BRISK_HIP_EINVAL, "apply_corrections: more rows than one launch covers");
        u64 bad = 0;
        if (n_reads) {
            if ((rc = ensure(h, h->corr_tmp, kCorrHead))) return rc;
            unsigned long long* d_flag = (unsigned long long*)h->corr_tmp.p + 8;
            HIPCHK(h, hipMemsetAsync(d_flag, 0xff, 8, h->stream));
            hipLaunchKernelGGL(k_correct_row_check, dim3(nblocks(n_corr, 256)), dim3(256), 0, h->stream, (const CorrectRow*)d_corr, n_corr, d_packed, d_starts, n_reads, d_flag);
            if ((rc = launch_check(h, "k_correct_row_check"))) return rc;
            HIPCHK(h, hipMemcpyAsync(&bad, d_flag, 8, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        if (bad != ~0ull)
            return fail(h, BRISK_HIP_EINVAL, "apply_corrections: row " + std::to_string(bad) + " of the correction table names a read >= n_reads or a pos beyond its read, its `from` is not the base that is there, its `to` is `from` or no code, or it does not lie behind the row before it in (read, pos)");
    }
    const u64 n_words = (last + 15) / 16;
    if (out_cap_words < n_words + 2)
        return fail(h, BRISK_HIP_ECAPACITY, "apply_corrections: " + std::to_string(last) + " nucleotides need " + std::to_string(n_words + 2) + " words, out_cap_words is " + std::to_string(out_cap_words));
    if (!n_reads) {
        HIPCHK(h, hipMemsetAsync(d_out_packed, 0, 8, h->stream));
    } else if ((rc = correct_apply_impl(h, d_packed, d_starts, (const CorrectRow*)d_corr, n_corr, n_words, d_out_packed, "apply_corrections"))) {
        return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_correct_packed(brisk_hip_index* h, const uint32_t* d_packed, const uint64_t* d_starts, uint64_t n_reads, uint32_t solid_min, uint32_t min_cover,
                                       uint32_t* d_out_packed, uint64_t out_cap_words, brisk_hip_correction* d_out_corrections, uint64_t corr_cap, brisk_hip_correct_stats* stats) {
    if (!h) return BRISK_HIP_EINVAL;
    if (int wrc = need_whole_index(h, "correct_packed")) return wrc;
    if (!stats || (n_reads && (!d_packed || !d_starts))) return fail(h, BRISK_HIP_EINVAL, "correct_packed: null pointer");
    if (!d_out_packed && out_cap_words) return fail(h, BRISK_HIP_EINVAL, "correct_packed: out_cap_words without d_out_packed");
    if (!d_out_corrections && corr_cap) return fail(h, BRISK_HIP_EINVAL, "correct_packed: corr_cap without d_out_corrections");
    u32 c = 0;
    if (int crc = check_min_cover(h, min_cover, "correct_packed", &c)) return crc;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    int rc;
    memset(stats, 0, sizeof(*stats));
    stats->n_reads = n_reads;
    u64 last = 0;
    if (n_reads) {
        u64 n_nts = 0;
        if ((rc = split_check_table(h, d_starts, n_reads, "correct_packed", true, &n_nts))) return rc;
        HIPCHK(h, hipMemcpyAsync(&last, d_starts + n_reads, 8, hipMemcpyDeviceToHost, h->stream));
        // a sibling of brisk_hip_split_packed's loop: a batch's slots into kout_tmp, and its corrections instead of its fragments
        const u64 batch = profile_batch_limit(h);
        for (u64 r0 = 0; r0 < n_reads; r0 += batch) {
            const u64 nb = std::min<u64>(batch, n_reads - r0);
            u64 ns = 0;
            if ((rc = count_kmers(h, d_starts + r0, nb, &ns))) return rc;
            if (ns) {
                if ((rc = ensure(h, h->kout_tmp, ns * 2))) return rc;
                HIPCHK(h, hipMemsetAsync(h->kout_tmp.p, 0, ns * 2, h->stream));
                if ((rc = kmers_packed_impl(h, d_packed, d_starts + r0, nb, (uint16_t*)h->kout_tmp.p, ns))) return rc;
            }
            if ((rc = correct_batch(h, d_packed, (const uint16_t*)h->kout_tmp.p, d_starts + r0, nb, ns, r0, solid_min, c, stats))) return rc;
        }
        if ((rc = check_device_flags(h))) return rc;
    }
    const u64 nc = stats->n_corrected, n_words = (last + 15) / 16;
    if (d_out_corrections && corr_cap < nc) return fail(h, BRISK_HIP_ECAPACITY, "correct_packed: " + std::to_string(nc) + " corrections, corr_cap is " + std::to_string(corr_cap));
    if (d_out_packed && out_cap_words < n_words + 2)
        return fail(h, BRISK_HIP_ECAPACITY, "correct_packed: " + std::to_string(last) + " nucleotides need " + std::to_string(n_words + 2) + " words, out_cap_words is " + std::to_string(out_cap_words));
    if (d_out_packed) {
        if (!n_reads) HIPCHK(h, hipMemsetAsync(d_out_packed, 0, 8, h->stream));
        else if ((rc = correct_apply_impl(h, d_packed, d_starts, (const CorrectRow*)h->corr_tab.p, nc, n_words, d_out_packed, "correct_packed"))) return rc;
    }
    if (d_out_corrections && nc) HIPCHK(h, hipMemcpyAsync(d_out_corrections, h->corr_tab.p, nc * 16, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BRISK_HIP_OK;
}

BRISK_API int brisk_hip_correct_reads(brisk_hip_index* h, const char* bases, const uint64_t* offsets, uint64_t n_reads, uint32_t solid_min, uint32_t min_cover,
                                      brisk_hip_correction* out_corrections, uint64_t corr_cap, brisk_hip_correct_stats* stats) {
    if (!h) return BRISK_HIP_EINVAL;
    if (int wrc = need_whole_index(h, "correct_reads")) return wrc;
    if (!stats || (corr_cap && !out_corrections) || (n_reads && (!bases || !offsets))) return fail(h, BRISK_HIP_EINVAL, "correct_reads: null pointer");
    u32 c = 0;
    if (int crc = check_min_cover(h, min_cover, "correct_reads", &c)) return crc;
    for (u64 r = 0; r < n_reads; r++) {
        if (offsets[r + 1] < offsets[r]) return fail(h, BRISK_HIP_EINVAL, "read offsets do not ascend (offsets[i + 1] < offsets[i])");
        if (offsets[r + 1] - offsets[r] > 0xffffffffull) return fail(h, BRISK_HIP_EINVAL, "correct_reads: a read of 2^32 nucleotides or more does not fit the correction record");
    }
    memset(stats, 0, sizeof(*stats));
    stats->n_reads = n_reads;
    if (!n_reads) return BRISK_HIP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    std::lock_guard<std::recursive_mutex> call_lock(h->call_mu);
    if (int frc = enter(h)) return frc;
    // a sibling of profile_host_batches: a batch is uploaded and packed, its slots go to kout_tmp, and the stream is waited for before
    // the next batch's upload overwrites the packed stream that this one's kernels read
    const u64 saved = h->max_batch_reads;
    h->max_batch_reads = profile_batch_limit(h);
    int rc = for_each_host_batch(h, bases, offsets, n_reads, [&](u64 r0, u64 nr) -> int {
        int rc2;
        const u64 ns = host_slots(offsets, r0, r0 + nr, h->P.k);
        if (ns) {
            if ((rc2 = ensure(h, h->kout_tmp, ns * 2))) return rc2;
            HIPCHK(h, hipMemsetAsync(h->kout_tmp.p, 0, ns * 2, h->stream));
            if ((rc2 = kmers_packed_impl(h, (const u32*)h->packed_tmp.p, (const u64*)h->starts_tmp.p, nr, (uint16_t*)h->kout_tmp.p, ns))) return rc2;
        }
        if ((rc2 = correct_batch(h, (const u32*)h->packed_tmp.p, (const uint16_t*)h->kout_tmp.p, (const u64*)h->starts_tmp.p, nr, ns, r0, solid_min, c, stats))) return rc2;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return BRISK_HIP_OK;
    });
    h->max_batch_reads = saved;
    if (rc) return rc;
    if ((rc = check_device_flags(h))) return rc;
    const u64 nc = stats->n_corrected;
    if (corr_cap < nc) return fail(h, BRISK_HIP_ECAPACITY, "correct_reads: " + std::to_string(nc) + " corrections, corr_cap is " + std::to_string(corr_cap));
    if (nc) {
        HIPCHK(h, hipMemcpyAsync(out_corrections, h->corr_tab.p, nc * 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return BRISK_HIP_OK;
}

}  // extern "C"
