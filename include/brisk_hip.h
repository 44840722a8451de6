/*
 * brisk_hip.h -- C-ABI of the MI355X-native Brisk hot path (libbrisk_hip.so).
 *
 * The reference has no FFI layer: its boundary is the header-only C++ API
 * consumed by apps/counter.cpp.  This C-ABI is the boundary
 * between that host-side C++ (brisk_amd/include/Brisk.hpp, same names as the
 * reference's) and the HIP kernels.  Plain pointers and sizes only; no C++,
 * torch or HIP types appear in any signature.  Every entry point returns an
 * int status (BRISK_HIP_OK == 0) and never throws.
 *
 * Threads.  The reference lets any number of OpenMP threads call insert_superkmer /
 * get_superkmer at once under its lock stripes (brisk/Brisk.hpp:112-114,140-143,
 * brisk/DenseMenuYo.hpp:110-118; apps/counter.cpp:197-227,314-346).  Here the unit of
 * work is a batch, and a handle takes ONE call at a time (a per-handle lock inside the
 * library; one HIP stream per handle): any number of host threads may call any entry
 * points on one handle concurrently -- e.g. one thread streaming brisk_hip_insert_reads
 * batches while another issues brisk_hip_get_reads / brisk_hip_lookup -- and every call
 * runs against the index as left by a whole number of the other threads' completed
 * calls.  A concurrent get therefore observes whole batches only: never a partly
 * inserted batch, never a torn entry (a key without its count, a count updated for some
 * of a read's k-mers only).  Which batches it observes depends on timing, as in the
 * reference.  Calls on different handles are independent.  brisk_hip_last_error is the
 * one exception: it returns the handle's last message without taking the lock.
 *
 * Reference interface each entry point stands in for (file:line under the
 * reference tree):
 *   brisk_hip_create            Parameters ctor + Brisk ctor + DenseMenuYo ctor
 *                               (brisk/parameters.hpp:24-34, brisk/Brisk.hpp:47-52,
 *                                brisk/DenseMenuYo.hpp:104-138)
 *   brisk_hip_destroy           Brisk dtor (brisk/Brisk.hpp:57-59)
 *   brisk_hip_clear             `delete menu; menu = new DenseMenuYo` (what Brisk::reallocate does
 *                               to start over, brisk/Brisk.hpp:220-222): an empty index that keeps
 *                               its device memory reserved
 *   brisk_hip_reallocate        Brisk::reallocate (brisk/Brisk.hpp:202-224)
 *   brisk_hip_insert_reads      count_sequence loop: SuperKmerEnumerator::next +
 *                               Brisk::protect_data/insert_superkmer/unprotect_data +
 *                               the counter update (apps/counter.cpp:231-276,
 *                               brisk/Kmers.cpp:522-603, brisk/Brisk.hpp:123-161);
 *                               also the declared-but-undefined
 *                               Brisk::insert_sequence (brisk/Brisk.hpp:27)
 *   brisk_hip_get_reads / brisk_hip_get_packed
 *                               query_sequence (apps/counter.cpp:281-310) over
 *                               Brisk::get_superkmer (brisk/Brisk.hpp:102-118) /
 *                               Brisk::get_sequence (brisk/Brisk.hpp:28); _packed: reads and sums on the device
 *   brisk_hip_get_kmers / brisk_hip_get_kmers_packed
 *                               Brisk::get_sequence (brisk/Brisk.hpp:28: one DATA* per k-mer of the sequence;
 *                               declared, never defined) as Brisk::get_superkmer (brisk/Brisk.hpp:102-118) over
 *                               every vector SuperKmerEnumerator yields; _packed: reads and answers on the device
 *   brisk_hip_read_profile_reads / brisk_hip_read_profile_packed
 *                               no reference counterpart (the reference answers one k-mer or one super-k-mer at a time; khmer's
 *                               normalize-by-median and trim-low-abund are the usual tools): the answers of brisk_hip_get_kmers
 *                               reduced on the device to one abundance record per read
 *   brisk_hip_select_intervals / brisk_hip_extract_packed / brisk_hip_trim_packed / brisk_hip_trim_reads
 *                               no reference counterpart (khmer's trim-low-abund and normalize-by-median act on the abundances
 *                               that brisk_hip_read_profile_* measures): a profile record becomes a nucleotide interval of its
 *                               read, and the kept intervals a new packed stream, on the device
 *   brisk_hip_intake_ascii / brisk_hip_intake_reads / brisk_hip_insert_raw_reads
 *                               no reference counterpart as a library call: with min_qual == 0 they restate, in bulk and on the
 *                               device, clean_dna (apps/counter.cpp:130-169), which cuts a record at every byte that is not a
 *                               base; the quality cut is Jellyfish's --min-qual-char and KMC's handling of N
 *   brisk_hip_fragment_intervals / brisk_hip_pair_intervals / brisk_hip_compose_intervals / brisk_hip_extract_pairs_packed /
 *   brisk_hip_trim_pairs_packed / brisk_hip_trim_pairs_reads / brisk_hip_clean_pairs_ascii / brisk_hip_clean_pairs_reads
 *                               no reference counterpart; khmer's extract-paired-reads and Trimmomatic's paired mode are the usual
 *                               tools: paired-end reads kept in sync through intake, trim and extraction -- the pair decision is
 *                               taken over the mates' intervals, and intact pairs and singles leave as two packed streams
 *   brisk_hip_solid_runs / brisk_hip_extract_fragments_packed / brisk_hip_split_packed / brisk_hip_split_reads
 *                               no reference counterpart; Quake, BFC and khmer's trim-low-abund -V are the usual tools: a read is
 *                               cut at its weak k-mers and every run of solid k-mers leaves as a fragment of its own
 *   brisk_hip_weak_sites / brisk_hip_candidate_windows / brisk_hip_decide_sites / brisk_hip_apply_corrections /
 *   brisk_hip_correct_packed / brisk_hip_correct_reads
 *                               no reference counterpart; Quake and BFC are the usual tools: a run of weak k-mers that one
 *                               substitution explains names the nucleotide, the three other bases are tried there, and the read is
 *                               repaired, whole, when exactly one of them makes every k-mer of the run solid
 *   brisk_hip_lookup            Brisk::get (brisk/Brisk.hpp:64-69)
 *   brisk_hip_enumerate         Brisk::next / restart_kmer_enumeration
 *                               (brisk/Brisk.hpp:166-179, brisk/DenseMenuYo.hpp:476-521)
 *   brisk_hip_stats             Brisk::stats (brisk/Brisk.hpp:194-197,
 *                               brisk/DenseMenuYo.hpp:545-568)
 *   brisk_hip_memory_info / brisk_hip_insert_slack   no reference counterpart (Brisk::stats reports the process' peak RSS): the arena's bookkeeping
 *   brisk_hip_count_spectrum / brisk_hip_enumerate_range / brisk_hip_prune
 *                               no reference counterpart (Brisk::stats and Brisk::next are all it has): the abundance
 *                               spectrum, the entries of a count range, and the index without the entries outside one,
 *                               each one pass over the arena on the device
 *   brisk_hip_adjacency / brisk_hip_degree_spectrum / brisk_hip_prune_degrees
 *                               no reference counterpart (it answers for nodes only; assemblers and cuttlefish build this graph):
 *                               the index as the node set of a de Bruijn graph -- which of its eight possible neighbours every
 *                               entry has, the histogram of (left, right) degrees, and the index without the nodes of given degrees
 *   brisk_hip_merge / brisk_hip_intersect / brisk_hip_subtract / brisk_hip_compare
 *                               no reference counterpart (the reference holds one index; kmc_tools and jellyfish merge are
 *                               the usual tools): two indexes of one geometry combined on the device, partition by partition
 *   brisk_hip_joint_spectrum / brisk_hip_filter_joint
 *                               no reference counterpart (kat comp and Merqury's spectra-cn are the usual tools): the histogram
 *                               of (count in a, count in b) with "absent" a state of its own, and the index filtered by both counts
 *   brisk_hip_save / brisk_hip_load / brisk_hip_snapshot_info_read
 *                               no reference counterpart (the reference's index lives as long as its process; jellyfish and KMC
 *                               keep their databases on disk): the directory and the live entries, as stored, to a file and back
 *   brisk_hip_checksum          the next()+get() walk of verif_counts (apps/counter.cpp:90-126), reduced
 *                               to a digest on the device
 *   brisk_hip_scan_packed / brisk_hip_route_records / brisk_hip_insert_records
 *                               the same insert path cut at the super-k-mer
 *                               boundary (the vector<kmer_full> handed from
 *                               SuperKmerEnumerator::next to Brisk::insert_superkmer,
 *                               apps/counter.cpp:242-261) so that records can be
 *                               exchanged between GPUs (no reference counterpart:
 *                               the reference is single-process)
 *   brisk_hip_set_owner_cuts    no reference counterpart: which partition range each GPU of a sharded job owns
 *   brisk_hip_export_hist / brisk_hip_export_hist_add / brisk_hip_insert_records_hist
 *                               no reference counterpart: the per-partition record counts of a scan travel with
 *                               the records so that the owner need not count them again
 *   brisk_hip_scan_query / brisk_hip_route_tagged / brisk_hip_query_records
 *                               the query path (apps/counter.cpp:281-310, brisk/Brisk.hpp:102-118) cut at the
 *                               same boundary, for a get across bucket-range shards
 *   brisk_hip_scan_kmers / brisk_hip_record_kmers / brisk_hip_answer_records / brisk_hip_place_answers / brisk_hip_profile_slots
 *                               no reference counterpart (the reference is single-process): the per-k-mer get and the read profile cut
 *                               at the same boundary, for brisk_hip_get_kmers and brisk_hip_read_profile_* across bucket-range shards
 *   brisk_hip_scan_sequence     SuperKmerEnumerator ctor + next() until empty (brisk/Kmers.cpp:509-603)
 *   brisk_hip_upsert_kmers      Brisk::insert_superkmer (brisk/Brisk.hpp:123-147) minus the DATA pointers,
 *                               which the facade forms from the returned ids
 *   brisk_hip_find_kmers        Brisk::get_superkmer / Brisk::get (brisk/Brisk.hpp:64-69,102-118)
 *   brisk_hip_enumerate_ids     Brisk::next (brisk/Brisk.hpp:166-172)
 *   brisk_hip_pack_ascii        nuc2int (brisk/Kmers.cpp:442-444) applied in bulk
 *   brisk_hip_unpack_ascii      no reference counterpart (kmer2str, brisk/Kmers.cpp, prints one k-mer): the inverse of
 *                               brisk_hip_pack_ascii over a stretch of a packed stream
 *   brisk_hip_synth_reads       no reference counterpart (benchmark input,
 *                               SURVEY.md 8(d))
 *   brisk_hip_debug_order_keys  bfc_hash_64 + DecyclingSet::memDouble in bulk
 *   brisk_hip_debug_guard_count how many of them the exact fold decided
 *                               (brisk/hashing.cpp:8-19, brisk/Decycling.cpp:38-52); test hook
 */
#ifndef BRISK_HIP_H
#define BRISK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRISK_HIP_ABI_VERSION 4

enum {
    BRISK_HIP_OK = 0,
    BRISK_HIP_EINVAL = 1,       /* parameter contract violated (e.g. b > m, m even) */
    BRISK_HIP_EUNSUPPORTED = 2, /* valid for the reference but outside this library's envelope */
    BRISK_HIP_EHIP = 3,         /* a HIP runtime call failed; see brisk_hip_last_error */
    BRISK_HIP_ENOMEM = 4,       /* device or host allocation failed */
    BRISK_HIP_ECAPACITY = 5,    /* caller-provided output buffer too small */
    BRISK_HIP_ENODEVICE = 6,    /* no usable gfx950 device */
    BRISK_HIP_EIO = 7,          /* a snapshot file: open/read/write/rename failed, or the file ends early */
    BRISK_HIP_EFORMAT = 8       /* not a snapshot, unknown version, inconsistent sizes, digest mismatch */
};

typedef struct brisk_hip_index brisk_hip_index;

typedef struct brisk_hip_options {
    uint32_t struct_size;       /* sizeof(brisk_hip_options), for ABI growth */
    int32_t device;             /* HIP device ordinal */
    void *stream;               /* hipStream_t to run on, NULL: the library creates one */
    uint32_t part_bits;         /* log2(#partitions), at most 2b; 0: default (2^24, also when 2b < 24: see brisk_hip_layout.ext_bits).
                                 * The insert is at its best with 10-20 records (a few hundred k-mer instances) per partition
                                 * and call: 2^24 suits batches of 50 M reads on one index; a sharded job whose owners each
                                 * receive that much (N x 50 M reads per batch over N owners) wants 24 + log2(N); a job of ONE
                                 * smaller batch of short k-mers wants fewer (k31 m15 b14, 20 M reads: 2^22 -- two-word records of
                                 * nine k-mers leave 2^24 partitions with a dozen entries each; the k63 insert loses with fewer
                                 * than 2^24).  brisk_amd.exchange.suggest_part_bits states the rule bench.py uses */
    uint32_t owner_rank;        /* this process' rank among n_owners bucket-range owners */
    uint32_t n_owners;          /* 0 or 1: this index owns every bucket; at most 256 (else EUNSUPPORTED) */
    uint32_t minimizer_mode;    /* BRISK_HIP_MINIMIZER_REFERENCE (0, also what a caller passing the struct without this field gets -- the field
                                 * lies in what was padding between n_owners and arena_entries, so no other member moved and the
                                 * struct's size is what it was; count_mode stays the last member):
                                 * the reference's get_minimizer as executed -- at k > 32 its re-scan reads the low 64 bits of the
                                 * k-mer only (Kmers.cpp:371), the minimizer it leaves depends on how the read arrived there and on
                                 * the strand, and one canonical k-mer enters the index under several identities (kmer_s,
                                 * minimizer_idx), its count split among them.  BRISK_HIP_MINIMIZER_FULL: that one truncation
                                 * removed -- the re-scan of the k-mer at an expiry and of the (k - 1)-mer at a read's start see all
                                 * of it, whatever k is; the step rule, the tie rules over all k - m + 1 windows, the canonical-form
                                 * test as executed, the ignored close at a read's first k-mer and the identity (kmer_s,
                                 * minimizer_idx) are the reference's.  For k <= 32 both modes are one function and build the same
                                 * index bit for bit.  Any other value: EINVAL.  The mode is the index's for life, like count_mode:
                                 * brisk_hip_get_minimizer_mode reports it, snapshots carry it (header offset 116), brisk_hip_load
                                 * refuses a file of the other mode, every scan of the handle follows it (brisk_hip_scan_sequence and
                                 * entry-id indexes included; upsert, find and lookup take identities from the caller), and the two
                                 * handles of a set operation, a joint spectrum or filter, or brisk_hip_reallocate must agree in it
                                 * (EINVAL, the message names minimizer_mode). */
    uint64_t arena_entries;     /* initial entry capacity of the k-mer arena; 0: grow on demand */
    uint64_t max_batch_reads;   /* reads per internal scan batch; 0: default */
    uint32_t entry_ids;         /* 1: entry-id mode (per-call facade API): every entry gets a stable dense id in
                                 * insertion order and DATA lives with the caller, indexed by id; bulk count
                                 * entry points are refused on such an index */
    uint32_t immediate_inserts; /* 0: an insert call whose batch would leave the partitions nearly empty (fewer than ~24 M reads
                                 * at k=63 on 2^24 partitions) is scanned at once and its records inserted together with those of
                                 * the next such calls -- at the latest when any call other than an insert arrives (they all
                                 * complete pending inserts first), so no call ever sees an index without them; an error of
                                 * the deferred part (BRISK_HIP_ENOMEM) is returned by the call that completes it.  Streams
                                 * of 2 M-read batches go in 3x faster that way.  1: every insert call completes before it
                                 * returns. */
    uint32_t count_mode;        /* BRISK_HIP_COUNTS_WRAP (0, also what a caller passing the struct without this field gets): the
                                 * count byte wraps, first touch = 1, then ++ mod 256, as the reference's uint8_t counter.
                                 * BRISK_HIP_COUNTS_SATURATE: an entry's stored count is min(255, the number of times its identity
                                 * was inserted), whatever the batching, the deferral, the kernels that ran or the record layout:
                                 * 255 means "255 or more", and a present entry never has count 0.  Any other value: EINVAL, as is
                                 * SATURATE together with entry_ids (that DATA lives with the caller).  The mode is the index's
                                 * for life: brisk_hip_layout.count_mode reports it, snapshots carry it, and two handles of a set
                                 * operation or of brisk_hip_reallocate must agree in it. */
} brisk_hip_options;
enum { BRISK_HIP_COUNTS_WRAP = 0, BRISK_HIP_COUNTS_SATURATE = 1 };
enum { BRISK_HIP_MINIMIZER_REFERENCE = 0, BRISK_HIP_MINIMIZER_FULL = 1 };

/* ---- lifetime ----------------------------------------------------------- */
/* coef_table: the 4*m doubles of DecyclingSet(m) computed on the HOST with libm
 * (brisk/Decycling.cpp:7-13); the device never evaluates sin().  data_bytes must
 * be 1 (the counter app's uint8_t DATA).
 * The envelope: 1 <= b <= m < k <= 63, m odd and at most 31, k - b >= 4 (EINVAL otherwise); b <= 16 and an entry key
 * [routing bits | compacted k-mer : 2(k-b) | idx' : 6] of at most 128 bits (EUNSUPPORTED otherwise).  k - b < 4 is EINVAL, not
 * EUNSUPPORTED: the reference itself cannot build such an index (SuperKmerLight.hpp:62 makes a mask of 2 (k - b) - 8 bits,
 * which underflows and aborts), so no result exists to agree with. */
int brisk_hip_create(brisk_hip_index **out, uint8_t k, uint8_t m, uint8_t b, uint32_t data_bytes,
                     const double *coef_table, const brisk_hip_options *opt);
int brisk_hip_destroy(brisk_hip_index *h);
/* back to the empty index; device memory stays reserved for the next job */
int brisk_hip_clear(brisk_hip_index *h);
const char *brisk_hip_last_error(const brisk_hip_index *h);
int brisk_hip_sync(brisk_hip_index *h);
uint32_t brisk_hip_abi_version(void);

/* derived constants (mirrors brisk/parameters.hpp:24-34) */
typedef struct brisk_hip_layout {
    uint32_t k, m, b, m_reduc, compacted_size, allocated_bytes;
    uint32_t record_words;      /* u64 words per super-k-mer record (incl. header word) */
    uint32_t part_bits;         /* log2(#partitions) */
    uint32_t n_owners, owner_rank;
    uint32_t ext_bits;          /* a record's routing id (header bits 0..31) = bucket id << ext_bits | ext_bits more bits: first
                                 * more of the same hashed minimizer, then (lowest) cls_bits of class; 0 when 2b >= 24 or
                                 * part_bits was given: the bucket id itself */
    uint32_t cls_bits;          /* 2m < 24 only: the lowest cls_bits of a routing id are min(minimizer_idx / cls_width,
                                 * 2^cls_bits - 1) of the record's k-mers, and a super-k-mer spanning several classes is
                                 * scanned into one record per class (each a valid super-k-mer of the same bucket) */
    uint32_t cls_width;
    uint32_t count_mode;        /* brisk_hip_options.count_mode of the handle: BRISK_HIP_COUNTS_WRAP or BRISK_HIP_COUNTS_SATURATE */
} brisk_hip_layout;
int brisk_hip_get_layout(const brisk_hip_index *h, brisk_hip_layout *out);
/* brisk_hip_options.minimizer_mode of the handle: BRISK_HIP_MINIMIZER_REFERENCE or BRISK_HIP_MINIMIZER_FULL.  (A call of its own:
 * brisk_hip_layout has no struct_size to grow behind and no padding to grow into.)  EINVAL on a null argument. */
int brisk_hip_get_minimizer_mode(const brisk_hip_index *h, uint32_t *out);

/* ---- bulk count (DATA = uint8_t counter: first touch = 1, then ++ mod 256; with BRISK_HIP_COUNTS_SATURATE: ++ up to 255) -- */
/* HOST buffers: `bases` = concatenated sequences, `offsets[n_reads+1]`.  Sequences
 * must be clean ([ACGTacgt]; the N-splitting of counter.cpp:130-169 is the caller's);
 * sequences shorter than k are skipped (counter.cpp:233-235).  A large batch is taken in
 * pieces: a dozen host threads turn the bytes into the 2-bit stream (nuc2int, Kmers.cpp:442-444)
 * while they stage them into pinned memory, and the scan of one piece runs under the upload of
 * the next (environment: BRISK_UPLOAD_LANES, BRISK_PIPE_PIECES, BRISK_UPLOAD_PIPELINE=0,
 * BRISK_HOST_PACK=0 for ASCII over PCIe and k_pack_ascii on arrival).  Non-base bytes are not
 * detected here (each is counted as the base its bits 1-2 spell): brisk_hip_insert_raw_reads is
 * the entry point for input that may hold them. */
int brisk_hip_insert_reads(brisk_hip_index *h, const char *bases, const uint64_t *offsets, uint64_t n_reads);

/* DEVICE buffers: 2-bit packed stream (16 nts per u32, first nt in the top bits;
 * A0 C1 T2 G3) and per-read start offsets in nucleotides, starts[n_reads+1].
 * d_packed must be readable 8 bytes past the last used word. */
int brisk_hip_insert_packed(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads);

/* ---- bulk query ---------------------------------------------------------- */
/* per_read_sum[r] = sum of the counts of the read's k-mers that are present,
 * with query_sequence's quirk: enumeration of a read stops at the first
 * super-k-mer after the first whose minimizer value is 0 (counter.cpp:304-306). */
int brisk_hip_get_reads(brisk_hip_index *h, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                        uint64_t *per_read_sum);
/* the same with reads and sums resident on the device (layout of brisk_hip_insert_packed; d_per_read_sum[n_reads]) */
int brisk_hip_get_packed(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                         uint64_t *d_per_read_sum);

/* Per-k-mer get: the count at every k-mer position of every read.  Reads as for brisk_hip_get_reads (clean sequences; a read
 * shorter than k contributes nothing).  Read r owns max(0, len_r - k + 1) slots, starting at base_r = the sum of the earlier
 * reads' slots (64-bit: 50 M reads at k = 63 are 4.4 G slots); slot base_r + i is the k-mer that starts at nucleotide i of read
 * r.  A slot holds 0 when the k-mer is absent and 0x100 | count when it is present (the count is kept mod 256, so a present
 * k-mer can have count 0: the 0x100 bit says it is there; in a saturating index, brisk_hip_options.count_mode, a present k-mer's
 * count is 1..255 and 255 means "255 or more").  A k-mer is looked up under the (kmer_s, minimizer_idx) that
 * SuperKmerEnumerator gives it while scanning the WHOLE read -- the identity brisk_hip_insert_reads stored; minimizer ties make
 * it depend on the context, so it is not always the identity of the k-mer enumerated on its own.  Every slot of every read is
 * answered: the stop of brisk_hip_get_reads at a returned minimizer of 0 (counter.cpp:304-306) belongs to that per-read sum,
 * not to get_superkmer.  Pending deferred inserts are completed first.  The answer does not depend on max_batch_reads, on how
 * the call is batched or on which kernels run.  EINVAL on a sharded index (n_owners > 1) and on an entry-id index.  Across shards the
 * same slots come from brisk_hip_scan_kmers / _route_tagged / _record_kmers / _answer_records / _place_answers (below). */
/* HOST reads (layout of brisk_hip_get_reads); out[cap] HOST.  BRISK_HIP_ECAPACITY, nothing written, if cap < total slots. */
int brisk_hip_get_kmers(brisk_hip_index *h, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                        uint16_t *out, uint64_t cap);
/* DEVICE reads (layout of brisk_hip_insert_packed); d_out DEVICE, sized to the total slots. */
int brisk_hip_get_kmers_packed(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                               uint16_t *d_out);

/* Per-read abundance profile: the answers of brisk_hip_get_kmers reduced, on the device, to one record per read (no reference
 * counterpart).  A slot is PRESENT when its k-mer is in the index (the 0x100 bit of get_kmers) and SOLID when it is present and its
 * stored count is >= solid_min.  Stored counts are mod 256: an entry whose count wrapped to 0 is present with count 0, and solid only
 * when solid_min == 0 (a saturating index, brisk_hip_options.count_mode, has no such entry: its counts stop at 255, which then
 * stands for "255 or more" in min_present, max_present, the medians and the sum); solid_min > 255 means that no slot is solid.  `median` is the lower median over ALL slots of the read, an
 * absent slot counting 0 (what digital normalisation compares with its cutoff); `median_present` leaves the absent slots out.  The
 * run is the longest stretch of consecutive solid slots, the FIRST one when several are equally long: nucleotides
 * [run_start, run_start + run_len + k - 1) of the read are covered by solid k-mers only (abundance trimming keeps them).
 * Semantics are those of brisk_hip_get_kmers: the same read layouts; a k-mer is looked up under the (kmer_s, minimizer_idx) that the
 * scan of the WHOLE read gives it; every slot is answered (the stop of brisk_hip_get_reads at a returned minimizer of 0 does not
 * apply); pending deferred inserts are completed first; the answer does not depend on max_batch_reads, on how the call is batched or
 * on which kernels run.  A read shorter than k gets the all-zero record.  EINVAL on a sharded index (n_owners > 1), on an entry-id
 * index, on offsets that do not ascend and on a read of more than 2^32 - 1 slots.  The slots never leave the library: they are
 * written for one internal batch at a time into scratch memory of the handle and reduced there, so device memory grows with a
 * batch's slots (2 bytes each; a batch is at most min(max_batch_reads, BRISK_PROFILE_BATCH = 2^24) reads), not with the call's, and
 * the caller never allocates a slot array.  Reads of more than BRISK_PROFILE_SEG slots (environment, read once per process;
 * default 4096) are reduced in segments of that many slots and their partial results folded in order; the record is the same.
 * Across shards the slots come from the round trip of brisk_hip_scan_kmers and brisk_hip_profile_slots reduces them (below). */
typedef struct brisk_hip_read_profile {   /* 32 bytes, little-endian, no padding */
    uint32_t n_kmers;        /* slots of the read: max(0, len - k + 1) */
    uint32_t n_present;      /* slots whose k-mer is in the index */
    uint32_t n_solid;        /* present and stored count >= solid_min */
    uint32_t run_start;      /* longest run of consecutive solid slots: first slot (nucleotide position) ... */
    uint32_t run_len;        /* ... and its length; the FIRST such run on ties; 0, 0 when n_solid == 0 */
    uint8_t  min_present;    /* smallest / largest stored count over present slots; 0, 0 when n_present == 0 */
    uint8_t  max_present;
    uint8_t  median;         /* lower median over ALL slots, an absent slot counting 0: sorted[(n_kmers - 1) / 2]; 0 when n_kmers == 0 */
    uint8_t  median_present; /* lower median over present slots only; 0 when n_present == 0 */
    uint64_t sum;            /* sum of the stored counts of present slots */
} brisk_hip_read_profile;
/* HOST reads (layout of brisk_hip_get_reads); out[n_reads] HOST: 32 bytes a read come back */
int brisk_hip_read_profile_reads(brisk_hip_index *h, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                                 uint32_t solid_min, brisk_hip_read_profile *out);
/* DEVICE reads (layout of brisk_hip_insert_packed); d_out[n_reads] DEVICE */
int brisk_hip_read_profile_packed(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                                  uint32_t solid_min, brisk_hip_read_profile *d_out);

/* ---- read extraction: trim and filter by abundance profile (no reference counterpart) ---- */
/* A rule turns a profile record into an interval of its read, in nucleotides; len == 0 means that the read is dropped.
 *   BRISK_HIP_SELECT_SOLID_RUN  [run_start, run_start + run_len + k - 1) when run_len >= 1 (the nucleotides that the first longest run
 *                               of solid k-mers covers: abundance trimming), else dropped
 *   BRISK_HIP_SELECT_MEDIAN     the whole read [0, n_kmers + k - 1) when lo <= median <= hi (digital normalisation keeps a read whose
 *                               median is below its cut-off; a screen keeps one whose median is at least 1), else dropped
 *   BRISK_HIP_SELECT_PRESENT    the whole read when lo * n_kmers <= 1000 * n_present <= hi * n_kmers (the share of the read's k-mers
 *                               that are in the index, in permille, 64-bit products), else dropped
 * For every kind: a read with n_kmers == 0 is dropped, and so is an interval shorter than max(min_len, k) nucleotides (and one of
 * 2^32 nucleotides or more, which the record cannot hold).  EINVAL: a null rule, struct_size < sizeof(brisk_hip_select_rule), an
 * unknown kind, lo > hi.  brisk_amd.intervals_from_profile is the same rule in numpy: the definition the tests compare with. */
typedef struct brisk_hip_read_interval { uint32_t start, len; } brisk_hip_read_interval; /* nucleotides of the read; len == 0: the read is dropped */
enum { BRISK_HIP_SELECT_SOLID_RUN = 0, BRISK_HIP_SELECT_MEDIAN = 1, BRISK_HIP_SELECT_PRESENT = 2 };
typedef struct brisk_hip_select_rule {
    uint32_t struct_size;
    uint32_t kind;
    uint32_t min_len;   /* kept interval must have at least this many nts; 0 means k */
    uint32_t lo, hi;    /* MEDIAN: lo <= record.median <= hi.  PRESENT: lo*n_kmers <= 1000*n_present <= hi*n_kmers (permille, 64-bit products) */
} brisk_hip_select_rule;
/* d_intervals[r] = the rule applied to d_profiles[r] (both DEVICE, n_reads each), with the handle's k.  Needs no index state: any
 * handle serves. */
int brisk_hip_select_intervals(brisk_hip_index *h, const brisk_hip_read_profile *d_profiles, uint64_t n_reads,
                               const brisk_hip_select_rule *rule, brisk_hip_read_interval *d_intervals);
/* The kept intervals of a packed stream as a new packed stream, all on the device.  Input: the layout of brisk_hip_insert_packed and
 * d_intervals[n_reads].  Output, in the same layout: 16 nts per u32, first nt in the top bits; the kept reads (len > 0) concatenated
 * at nucleotide granularity in input order, dropped reads absent; d_out_starts[0 .. n_out] ascending from 0 (room for n_reads + 1);
 * d_out_index[j] (room for n_reads; may be NULL) = the index, in the input, of kept read j; the unused low bits of the last word zero
 * and the two words after it zero ("readable 8 bytes past the last used word").  *n_out_reads and *n_out_nts (HOST) receive the
 * counts (64-bit: 50 M reads of 150 bp are 7.5 G nucleotides).  out_cap_words >= ceil(n_out_nts / 16) + 2 is required -- an output
 * of as many words as the input stream has, its two readable words included, always suffices -- else BRISK_HIP_ECAPACITY, nothing
 * written (the counts are: the call can be repeated with room).  EINVAL, nothing written: an interval with start + len beyond its
 * read (found on the device; the message names the first such read), a read table that does not ascend, null pointers.  The output
 * may not overlap the input.  Every output word is stored once by a plain vector store; no source word past the last one that
 * holds a kept nucleotide is read.  Needs no index state: works on any handle (sharded and entry-id ones included), on the handle's
 * stream and under its lock; it returns when the output is complete. */
int brisk_hip_extract_packed(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                             const brisk_hip_read_interval *d_intervals,
                             uint32_t *d_out_packed, uint64_t out_cap_words, uint64_t *d_out_starts /* n_reads+1 room */,
                             uint64_t *d_out_index /* n_reads room, may be NULL: original index of each kept read */,
                             uint64_t *n_out_reads, uint64_t *n_out_nts /* HOST */);
/* brisk_hip_read_profile_packed, the rule, brisk_hip_extract_packed in one call: profile, trim, and the trimmed reads are ready for
 * brisk_hip_insert_packed / _get_packed / _read_profile_packed without leaving the device.  The records (one internal batch at a
 * time) and the intervals (8 bytes a read) live in scratch memory of the handle.  trim_reads takes HOST reads (layout of
 * brisk_hip_get_reads) and returns only the intervals, out[n_reads] HOST: the caller slices its own strings.  Both inherit
 * brisk_hip_read_profile_*: pending deferred inserts are completed first; EINVAL on a sharded index, on an entry-id index, on offsets
 * that do not ascend; the answer does not depend on max_batch_reads, BRISK_PROFILE_BATCH, BRISK_PROFILE_SEG or on which kernels run.
 * Across shards: brisk_hip_profile_slots over the slots of the brisk_hip_scan_kmers round trip, then select_intervals and extract_packed. */
int brisk_hip_trim_packed(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                          uint32_t solid_min, const brisk_hip_select_rule *rule,
                          uint32_t *d_out_packed, uint64_t out_cap_words, uint64_t *d_out_starts, uint64_t *d_out_index,
                          uint64_t *n_out_reads, uint64_t *n_out_nts);
int brisk_hip_trim_reads(brisk_hip_index *h, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                         uint32_t solid_min, const brisk_hip_select_rule *rule, brisk_hip_read_interval *out /* HOST, n_reads */);

/* ---- raw read intake: N and quality cuts on the device (kernels: brisk_intake.hip) ----------------------------------------- */
/* Input: `bases`, bytes of any value; `quals`, bytes aligned with them, or NULL; offsets[n_reads + 1], ascending byte offsets (read r
 * is [offsets[r], offsets[r + 1]); empty reads are allowed).  A byte is VALID when it is one of ACGTacgt and either min_qual == 0 or
 * its quality byte >= qual_base + min_qual (unsigned compare).  A FRAGMENT is a maximal run of valid bytes inside one read (a run
 * never crosses a read boundary) of at least L = max(min_len, k) bytes, k the handle's.  Fragments are ordered by read, then by
 * position.  With min_qual == 0 the fragments of a record body are the sequences of at least k nucleotides that clean_dna
 * (counter.cpp:130-169) cuts it into.  brisk_amd.fragments_from_reads is the same rule in numpy: the definition the tests compare with.
 * EINVAL: a null rule, a short struct_size, min_qual > 93, a qual_base other than 0 / 33 / 64, min_qual > 0 with NULL quals, a read of
 * 2^32 bytes or more, offsets that do not ascend. */
typedef struct brisk_hip_intake_rule {
    uint32_t struct_size;
    uint32_t min_len;    /* a fragment has at least max(min_len, k) nucleotides; 0 means k */
    uint32_t min_qual;   /* 0..93; 0: no quality cut, quals may be NULL */
    uint32_t qual_base;  /* 33 or 64; 0 means 33 */
} brisk_hip_intake_rule;
typedef struct brisk_hip_fragment { uint64_t read; uint32_t start, len; } brisk_hip_fragment; /* 16 bytes; start is relative to the read */
typedef struct brisk_hip_intake_stats {
    uint64_t n_reads;
    uint64_t n_reads_kept;  /* reads with at least one fragment */
    uint64_t n_fragments;
    uint64_t n_bases_in;    /* offsets[n_reads] - offsets[0] */
    uint64_t n_nts;         /* bytes inside fragments */
    uint64_t n_cut_base;    /* bytes that are not one of the eight letters */
    uint64_t n_cut_qual;    /* bytes that are a base but below the quality threshold */
    uint64_t n_short;       /* valid bytes in runs shorter than L */
} brisk_hip_intake_stats;   /* n_bases_in == n_nts + n_cut_base + n_cut_qual + n_short, always */
#define BRISK_HIP_INTAKE_BLOCK 4096 /* input bytes per thread block of the intake kernels: where a run's begin is carried across */
/* Everything on the DEVICE except `rule` and `stats`.  Output: the layout of brisk_hip_insert_packed -- 16 nts per u32, first nt in
 * the top bits, A0 C1 T2 G3, lower case packed as upper; the fragments concatenated at nucleotide granularity;
 * d_out_starts[0 .. n_fragments] ascending from 0; d_out_frags[j] (may be NULL) says where fragment j came from; the unused low bits
 * of the last word zero and the two words after it zero.  d_out_packed == NULL with out_cap_words == 0: the table and the stats only.
 * BRISK_HIP_ECAPACITY when frag_cap < n_fragments or out_cap_words < ceil(n_nts / 16) + 2: nothing is written to the device outputs,
 * *stats is filled, and the call can be repeated with room.  frag_cap = n_bases_in / L and out_cap_words = ceil(n_bases_in / 16) + 2
 * always suffice.  Needs no index state: works on any handle (sharded and entry-id ones included), on the handle's stream and under
 * its lock; it returns when the output is complete.  No byte outside [offsets[0], offsets[n_reads]) of either input is read; d_bases
 * and d_quals may have any alignment.  The output may not overlap the inputs.  Every output word and table row is stored once, by a
 * plain store.  Scratch memory of the handle: 4 bytes per 16 input bytes, 32 bytes per fragment. */
int brisk_hip_intake_ascii(brisk_hip_index *h, const char *d_bases, const char *d_quals /* NULL ok */, const uint64_t *d_offsets,
                           uint64_t n_reads, const brisk_hip_intake_rule *rule,
                           uint32_t *d_out_packed, uint64_t out_cap_words, uint64_t *d_out_starts /* frag_cap + 1 room */,
                           brisk_hip_fragment *d_out_frags /* frag_cap room, may be NULL */, uint64_t frag_cap,
                           brisk_hip_intake_stats *stats /* HOST */);
/* HOST reads in, the fragment table out (out_frags[frag_cap], HOST): the caller slices its own strings, as with brisk_hip_trim_reads.
 * Taken in pieces of whole reads (BRISK_INTAKE_PIECE).  ECAPACITY when frag_cap < n_fragments: *stats is filled for the whole call, so
 * it can be repeated with room; unlike the device call, out_frags is then partly written (the rows of the leading pieces that fit). */
int brisk_hip_intake_reads(brisk_hip_index *h, const char *bases, const char *quals /* NULL ok */, const uint64_t *offsets,
                           uint64_t n_reads, const brisk_hip_intake_rule *rule, brisk_hip_fragment *out_frags, uint64_t frag_cap,
                           brisk_hip_intake_stats *stats);
/* HOST reads are uploaded as they are, cut on the device, and the fragments inserted through the path brisk_hip_insert_packed takes
 * (deferral of small batches included).  The index afterwards is bit for bit the one brisk_hip_insert_reads builds from the
 * fragments' strings, however the call is split: a large call is taken in pieces of whole reads, at least one read per piece
 * (BRISK_INTAKE_PIECE=<bytes> sets the piece size; a test hook, read when the handle is created).  A piece's raw bytes, fragment
 * table and packed stream live in scratch memory of the handle.  Refused exactly where brisk_hip_insert_reads is (a sharded or
 * entry-id index), with the same code.  This sends 8 bits per nucleotide over the host link (16 with qualities) where
 * brisk_hip_insert_reads sends 2: clean input should stay there.  stats may be NULL. */
int brisk_hip_insert_raw_reads(brisk_hip_index *h, const char *bases, const char *quals /* NULL ok */, const uint64_t *offsets,
                               uint64_t n_reads, const brisk_hip_intake_rule *rule, brisk_hip_intake_stats *stats);

/* ---- paired-end reads: mates kept in sync through intake, trim and extract (no reference counterpart; kernels: brisk_pairs.hip) ---- */
/* A paired stream is INTERLEAVED: reads 2p and 2p + 1 are mates 1 and 2 of pair p, and n_reads is even.  After any step a read is
 * kept when its interval has len > 0.  A pair is in one of four states -- both mates kept (intact), only mate 1, only mate 2,
 * neither -- and the surviving mate of a broken pair is a SINGLE.  Nothing else encodes the state of a pair: it is always readable
 * from its two intervals.  brisk_amd.intervals_from_fragments, pair_intervals, compose_intervals and split_pairs are the same four
 * definitions in numpy: what the tests compare with. */
/* d_intervals[r] (DEVICE, n_reads rows, every one written) = {start, len} of the first longest fragment of read r in an intake
 * fragment table (d_frags[n_frags], DEVICE: ordered by read, then by position, as brisk_hip_intake_ascii writes it), {0, 0} when the
 * read has none.  EINVAL, nothing written: a row with read >= n_reads or a row that stands before its predecessor (found on the
 * device; the message names the first such row).  n_frags == 0 is valid.  Needs no index state: any handle serves. */
int brisk_hip_fragment_intervals(brisk_hip_index *h, const brisk_hip_fragment *d_frags, uint64_t n_frags, uint64_t n_reads,
                                 brisk_hip_read_interval *d_intervals);
/* The pair decision.  d_each: what a rule keeps of every read judged alone; d_whole: what the read would be if kept uncut.
 *   BRISK_HIP_PAIR_EACH  out = each: mates are judged separately, singles can arise
 *   BRISK_HIP_PAIR_ALL   a pair keeps both `each` intervals when both have len > 0, else both become {0, 0}
 *   BRISK_HIP_PAIR_ANY   when either mate's `each` has len > 0 both mates get their `whole` interval (a mate whose `whole` has
 *                        len 0 stays dropped), else both become {0, 0}
 * d_whole is required for ANY and ignored otherwise.  EINVAL: odd n_reads, an unknown mode, ANY with d_whole NULL.  d_out may be
 * d_each.  All DEVICE, n_reads rows each.  Needs no index state. */
enum { BRISK_HIP_PAIR_EACH = 0, BRISK_HIP_PAIR_ALL = 1, BRISK_HIP_PAIR_ANY = 2 };
int brisk_hip_pair_intervals(brisk_hip_index *h, const brisk_hip_read_interval *d_each, const brisk_hip_read_interval *d_whole /* NULL ok unless ANY */,
                             uint64_t n_reads, uint32_t pair_mode, brisk_hip_read_interval *d_out);
/* Two cuts chained.  d_outer[n_reads]: the first cut, over the input reads; d_inner[n_kept]: a second cut, over the reads that the
 * first one kept; d_index[n_kept] (ascending, as brisk_hip_extract_packed writes it): the input read behind kept read j.
 * d_out[d_index[j]] = {outer.start + inner[j].start, inner[j].len} ({0, 0} when inner[j].len == 0); every other row of d_out is
 * {0, 0}; all n_reads rows are written.  EINVAL, nothing written: inner[j] leaves outer (inner.start + inner.len > outer.len) or
 * d_index[j] >= n_reads (found on the device; the message names the first such row j), or an index that does not ascend.  d_out
 * may not overlap the inputs.  All DEVICE.  Needs no index state. */
int brisk_hip_compose_intervals(brisk_hip_index *h, const brisk_hip_read_interval *d_outer, uint64_t n_reads,
                                const brisk_hip_read_interval *d_inner, const uint64_t *d_index, uint64_t n_kept,
                                brisk_hip_read_interval *d_out);
typedef struct brisk_hip_pair_counts {
    uint64_t n_pairs_in;       /* n_reads / 2 */
    uint64_t n_pairs_kept;     /* both mates kept */
    uint64_t n_single_first;   /* only mate 1 kept */
    uint64_t n_single_second;  /* only mate 2 kept */
    uint64_t n_pairs_dropped;  /* neither kept */
    uint64_t n_nts_pairs;      /* nucleotides of the pairs stream */
    uint64_t n_nts_singles;    /* nucleotides of the singles stream */
    uint64_t reserved;         /* 0 */
} brisk_hip_pair_counts;       /* n_pairs_in == n_pairs_kept + n_single_first + n_single_second + n_pairs_dropped, always */
/* brisk_hip_extract_packed for an interleaved stream, twice: the PAIRS output is, by definition, extract_packed over the intervals
 * of intact pairs (every other row {0, 0}), so it is interleaved again -- d_pairs_index[2j] + 1 == d_pairs_index[2j + 1]; the
 * SINGLES output is extract_packed over the intervals of singles.  Each output has the layout, the room rules (out_cap_words >=
 * ceil(nts / 16) + 2, starts n_reads + 1, index n_reads or NULL) and the guarantees stated there.  The four singles arguments may
 * all be NULL / 0: singles are then counted and dropped.  *counts (HOST) is filled whenever the intervals are valid.
 * BRISK_HIP_ECAPACITY when either output is too small: nothing is written to either, *counts is filled, and the call can be
 * repeated with room.  EINVAL exactly where brisk_hip_extract_packed gives it, and on odd n_reads.  The two masked tables live in
 * scratch memory of the handle (16 bytes a read).  Needs no index state: works on any handle. */
int brisk_hip_extract_pairs_packed(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                                   const brisk_hip_read_interval *d_intervals,
                                   uint32_t *d_pairs_packed, uint64_t pairs_cap_words, uint64_t *d_pairs_starts, uint64_t *d_pairs_index,
                                   uint32_t *d_singles_packed, uint64_t singles_cap_words, uint64_t *d_singles_starts, uint64_t *d_singles_index,
                                   brisk_hip_pair_counts *counts /* HOST */);
/* brisk_hip_trim_packed for clean, packed, interleaved reads: the profiles as trim_packed takes them, the rule gives `each`, for
 * BRISK_HIP_PAIR_ANY `whole` comes from the same profiles (the whole read [0, n_kmers + k - 1), dropped below max(rule.min_len, k)
 * nucleotides), then the pair decision and brisk_hip_extract_pairs_packed.  ANY with BRISK_HIP_SELECT_SOLID_RUN means "either mate
 * has a solid run: keep both whole".  Refusals and the independence of the answer from batching are those of brisk_hip_trim_packed;
 * EINVAL also on odd n_reads and an unknown pair_mode.  trim_pairs_reads takes HOST reads and returns the intervals after the pair
 * decision, out[n_reads] HOST, and the counts: the caller slices its own strings, as with brisk_hip_trim_reads. */
int brisk_hip_trim_pairs_packed(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                                uint32_t solid_min, const brisk_hip_select_rule *rule, uint32_t pair_mode,
                                uint32_t *d_pairs_packed, uint64_t pairs_cap_words, uint64_t *d_pairs_starts, uint64_t *d_pairs_index,
                                uint32_t *d_singles_packed, uint64_t singles_cap_words, uint64_t *d_singles_starts, uint64_t *d_singles_index,
                                brisk_hip_pair_counts *counts /* HOST */);
int brisk_hip_trim_pairs_reads(brisk_hip_index *h, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                               uint32_t solid_min, const brisk_hip_select_rule *rule, uint32_t pair_mode,
                               brisk_hip_read_interval *out /* HOST, n_reads */, brisk_hip_pair_counts *counts /* HOST */);
/* Raw interleaved reads (bytes of any value, optional qualities: the input of brisk_hip_intake_ascii) to clean pairs and singles,
 * one interval per raw read.  The intake table is built (only the table); the first longest fragment of a read is the read's (iv1,
 * brisk_hip_fragment_intervals); the raw bytes are packed into scratch memory (a byte that is no base packs to some code and always
 * lies outside iv1).  select == NULL: each = iv1, no abundance stage, any handle serves.  Otherwise the one-fragment-per-read stream
 * is extracted, profiled with solid_min, cut by the select rule, and the cut composed back into the raw read's frame
 * (brisk_hip_compose_intervals): each; the handle must then be one that brisk_hip_trim_packed takes.  whole = iv1.  Then the pair
 * decision and brisk_hip_extract_pairs_packed from the packed raw stream.  d_out_intervals (DEVICE, n_reads rows, may be NULL)
 * receives the final intervals, relative to the raw reads; *stats the intake's; *counts the pairs'.  ECAPACITY as in
 * brisk_hip_extract_pairs_packed (d_out_intervals is then not written).  clean_pairs_reads takes HOST reads in pieces of whole
 * pairs (BRISK_INTAKE_PIECE) and returns the intervals, out[n_reads] HOST: the caller slices its own strings. */
int brisk_hip_clean_pairs_ascii(brisk_hip_index *h, const char *d_bases, const char *d_quals /* NULL ok */, const uint64_t *d_offsets,
                                uint64_t n_reads, const brisk_hip_intake_rule *intake, const brisk_hip_select_rule *select /* NULL ok */,
                                uint32_t solid_min, uint32_t pair_mode,
                                uint32_t *d_pairs_packed, uint64_t pairs_cap_words, uint64_t *d_pairs_starts, uint64_t *d_pairs_index,
                                uint32_t *d_singles_packed, uint64_t singles_cap_words, uint64_t *d_singles_starts, uint64_t *d_singles_index,
                                brisk_hip_read_interval *d_out_intervals /* may be NULL */,
                                brisk_hip_pair_counts *counts /* HOST */, brisk_hip_intake_stats *stats /* HOST */);
int brisk_hip_clean_pairs_reads(brisk_hip_index *h, const char *bases, const char *quals /* NULL ok */, const uint64_t *offsets,
                                uint64_t n_reads, const brisk_hip_intake_rule *intake, const brisk_hip_select_rule *select /* NULL ok */,
                                uint32_t solid_min, uint32_t pair_mode, brisk_hip_read_interval *out /* HOST, n_reads */,
                                brisk_hip_pair_counts *counts /* HOST */, brisk_hip_intake_stats *stats /* HOST */);

/* ---- read splitting: every solid run of a read as its own fragment (no reference counterpart; kernels: brisk_split.hip) ---- */
/* SLOT, PRESENT and SOLID mean what they mean in brisk_hip_read_profile: read r owns max(0, len_r - k + 1) slots, a slot is solid
 * when it is present and its stored count is >= solid_min (solid_min > 255: none is; solid_min == 0: every present slot is, one
 * whose count wrapped to 0 included).  A RUN is a maximal stretch of consecutive solid slots of one read: the last slot of read r and
 * the first slot of read r + 1 are neighbours in the slot array and never in one run.  A run of s slots that starts at slot i covers
 * nucleotides [i, i + s + k - 1) of its read, and is a FRAGMENT {read, start = i, len = s + k - 1} when s + k - 1 >= L = max(min_len,
 * k).  Fragments are ordered by read, then by start.  Two fragments of one read may OVERLAP by up to k - 2 nucleotides (the weak
 * k-mers between them share nucleotides with both): no solid k-mer is in two fragments and no weak k-mer is in any, but the output
 * can hold MORE nucleotides than the input -- an output as large as the input does not always suffice.  What always does:
 * frag_cap = (n_slots + n_reads) / 2 and out_cap_words = ceil((n_slots + frag_cap * (k - 1)) / 16) + 2; or ask first (a refused call
 * fills *stats).  For every read the first longest fragment at min_len = k is the interval of BRISK_HIP_SELECT_SOLID_RUN, and a
 * read has no fragment exactly when that interval has len 0.  brisk_amd.fragments_from_slots is the same rule in numpy: the
 * definition the tests compare with. */
typedef struct brisk_hip_split_stats {
    uint64_t n_reads;
    uint64_t n_reads_kept;  /* reads with at least one fragment */
    uint64_t n_fragments;
    uint64_t n_slots;
    uint64_t n_solid;       /* solid slots */
    uint64_t n_short;       /* solid slots in runs that cover fewer than L nucleotides */
    uint64_t n_nts_in;      /* starts[n_reads] - starts[0] */
    uint64_t n_nts_out;     /* the sum of len */
} brisk_hip_split_stats;    /* n_solid == (n_nts_out - n_fragments * (k - 1)) + n_short, always */
/* The fragment table of slots the caller holds (d_slots, DEVICE, read by d_starts exactly as brisk_hip_profile_slots reads them) ->
 * d_out_frags (DEVICE, frag_cap rows of room).  BRISK_HIP_ECAPACITY when frag_cap < n_fragments: nothing is written, *stats (HOST) is
 * filled, and the call can be repeated with room.  EINVAL: a read table that does not ascend, a read of 2^32 nucleotides or more,
 * null pointers.  Every row is stored once, by a plain vector store.  Needs no index state: works on any handle (sharded and
 * entry-id ones included; the slots of the brisk_hip_scan_kmers round trip can feed it).  Scratch memory of the handle: 8 bytes a
 * read, 4 bytes per 16 slots, 32 bytes a fragment. */
int brisk_hip_solid_runs(brisk_hip_index *h, const uint16_t *d_slots, const uint64_t *d_starts, uint64_t n_reads,
                         uint32_t solid_min, uint32_t min_len, brisk_hip_fragment *d_out_frags, uint64_t frag_cap,
                         brisk_hip_split_stats *stats /* HOST */);
/* The rows of a fragment table (d_frags[n_frags], DEVICE; any table, not only one written here) out of a packed stream, back to back
 * in table order, as a new packed stream in the layout of brisk_hip_extract_packed: d_out_starts[0 .. n_frags] ascending from 0, the
 * unused low bits of the last word zero and the two words after it zero.  Rows may overlap and may repeat a read.  EINVAL, nothing
 * written: a row with read >= n_reads, len == 0 or start + len beyond its read (found on the device; the message names the first
 * such row), a read table that does not ascend, null pointers.  BRISK_HIP_ECAPACITY, nothing written, *n_out_nts (HOST) filled: when
 * out_cap_words < ceil(n_nts / 16) + 2.  The output may not overlap the inputs.  Every output word is stored once by a plain vector
 * store.  Needs no index state: works on any handle. */
int brisk_hip_extract_fragments_packed(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                                       const brisk_hip_fragment *d_frags, uint64_t n_frags,
                                       uint32_t *d_out_packed, uint64_t out_cap_words, uint64_t *d_out_starts /* n_frags + 1 room */,
                                       uint64_t *n_out_nts /* HOST */);
/* brisk_hip_get_kmers_packed, brisk_hip_solid_runs and brisk_hip_extract_fragments_packed in one call: the fragments of a packed
 * stream as a packed stream that brisk_hip_insert_packed / _get_packed / _read_profile_packed take, without leaving the device.  The
 * slots exist for one internal batch at a time; the fragment table accumulates in scratch memory of the handle (16 bytes a
 * fragment, reads numbered as in the call) and the capacities are checked after the last batch: only then is anything copied or
 * gathered.  BRISK_HIP_ECAPACITY when frag_cap < n_fragments or out_cap_words < ceil(n_nts_out / 16) + 2: nothing is written to the
 * device outputs, *stats is filled, and the call can be repeated with room.  d_out_frags (frag_cap rows) may be NULL; d_out_starts
 * holds frag_cap + 1; d_out_packed == NULL with out_cap_words == 0: the table, the starts and the stats only.  Inherits
 * brisk_hip_trim_packed: pending deferred inserts are completed first; EINVAL on a sharded index, on an entry-id index, on offsets
 * that do not ascend (and on a read of 2^32 nucleotides or more); the answer does not depend on max_batch_reads,
 * BRISK_PROFILE_BATCH, BRISK_PROFILE_SEG or on which kernels run.  split_reads takes HOST reads (layout of brisk_hip_get_reads) and
 * returns only the table, out_frags[frag_cap] HOST, written when it fits: the caller slices its own strings. */
int brisk_hip_split_packed(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                           uint32_t solid_min, uint32_t min_len,
                           uint32_t *d_out_packed, uint64_t out_cap_words, uint64_t *d_out_starts /* frag_cap + 1 room */,
                           brisk_hip_fragment *d_out_frags /* frag_cap room, may be NULL */, uint64_t frag_cap,
                           brisk_hip_split_stats *stats /* HOST */);
int brisk_hip_split_reads(brisk_hip_index *h, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                          uint32_t solid_min, uint32_t min_len, brisk_hip_fragment *out_frags /* HOST */, uint64_t frag_cap,
                          brisk_hip_split_stats *stats /* HOST */);

/* ---- spectral read correction: isolated substitutions repaired (no reference counterpart; kernels: brisk_correct.hip) ---- */
/* SLOT, PRESENT and SOLID mean what they mean in brisk_hip_read_profile; read r has n = max(0, len - k + 1) slots.  A WEAK RUN is a
 * maximal stretch [i, i + w) of consecutive slots of one read that are not solid; it never crosses a read boundary.  Every weak run
 * falls into exactly one class, the tests applied in this order:
 *   whole   i == 0 && i + w == n: nothing solid anchors it
 *   long    w > k: more than one error
 *   short   (i > 0 && i + w < n && w < k): an interior run that an isolated substitution cannot explain; or w < C, where C =
 *           min_cover, 0 meaning k (allowed: 0..k, else EINVAL)
 *   else a SITE {read, pos, cover = w}: pos = i + w - 1 when a solid slot follows the run (i + w < n: interior runs of w == k, and
 *           runs at the read's left edge), pos = i + k - 1 when the run ends the read (i + w == n, i > 0).  A single substitution
 *           at nucleotide pos is the only one-error explanation of the run.
 * With min_cover = k only errors at least k - 1 nucleotides from both ends are attempted; smaller values reach towards the ends with
 * fewer witnesses.  Sites are ordered by read, then by pos; two sites of one read are at least k + 1 nucleotides apart, so no
 * site's window holds another site.  The WINDOW of a site is nucleotides [a, a + cover + k - 1) of its read, a = max(0, pos - k + 1):
 * its slots are exactly the run's.  A site has three CANDIDATES: the window with the base at pos replaced by one of the three other
 * 2-bit codes of the packed layout (A0 C1 T2 G3), in ascending code order.  Each candidate is looked up as a read of its own
 * (brisk_hip_get_kmers over the candidate stream): a k-mer is looked up under the (kmer_s, minimizer_idx) that the scan of the
 * WINDOW gives it, as brisk_hip_get_kmers does for whole reads (where that differs from its identity in the read the k-mer is absent
 * and the candidate fails: a true base can stay unresolved, a wrong one is never put in).  A candidate PASSES when all `cover` of its slots are solid at the
 * same solid_min.  Exactly one passes: the site is CORRECTED; two or three: AMBIGUOUS, and the read stays as it is there; none:
 * UNRESOLVED.  The OUTPUT is the input stream with the two bits of every corrected site replaced and nothing else changed: the word
 * count, the read table, the zero bits after the last nucleotide and the two readable words behind the stream are the input's.
 * Not covered: insertions, deletions and errors within k of each other (they leave long or short runs); iterating to a fixed point
 * (call it again on its output); qualities; sharded handles in the composed calls; FASTQ output.  brisk_amd.sites_from_slots and
 * corrections_from_candidates are the same rules in numpy: the definitions the tests compare with. */
typedef struct brisk_hip_site { uint64_t read; uint32_t pos, cover; } brisk_hip_site; /* 16 bytes; pos is relative to the read */
typedef struct brisk_hip_correction { uint64_t read; uint32_t pos; uint8_t from, to; uint16_t cover; } brisk_hip_correction; /* 16 bytes; from, to: packed codes */
typedef struct brisk_hip_correct_stats {
    uint64_t n_reads;
    uint64_t n_slots;
    uint64_t n_weak;        /* slots that are not solid */
    uint64_t n_runs;        /* weak runs: n_sites + n_skip_whole + n_skip_long + n_skip_short, always */
    uint64_t n_sites;       /* n_corrected + n_ambiguous + n_unresolved, always (calls that decide) */
    uint64_t n_skip_whole;
    uint64_t n_skip_long;
    uint64_t n_skip_short;
    uint64_t n_corrected;
    uint64_t n_ambiguous;
    uint64_t n_unresolved;
} brisk_hip_correct_stats;  /* 88 bytes */
/* The sites of slots the caller holds (d_slots, DEVICE, read by d_starts exactly as brisk_hip_solid_runs reads them) -> d_out_sites
 * (DEVICE, site_cap rows of room).  Fills every field of *stats (HOST) but the three decision counters.  BRISK_HIP_ECAPACITY when
 * site_cap < n_sites: nothing is written, *stats is filled, and the call can be repeated with room (what always suffices: a read of n
 * slots has at most (n + 1) / 2 weak runs).  EINVAL: min_cover > k, a read table that does not ascend, a read of 2^32 nucleotides
 * or more, null pointers.  Every row is stored once, by a plain vector store.  Needs no index state: works on any handle. */
int brisk_hip_weak_sites(brisk_hip_index *h, const uint16_t *d_slots, const uint64_t *d_starts, uint64_t n_reads,
                         uint32_t solid_min, uint32_t min_cover, brisk_hip_site *d_out_sites, uint64_t site_cap,
                         brisk_hip_correct_stats *stats /* HOST */);
/* The 3 * n_sites candidate windows of a site table (d_sites[n_sites], DEVICE; any table) as a packed stream in the layout of
 * brisk_hip_extract_packed, the substitution already in them: candidate c of site s is read 3 s + c of the output, and
 * d_out_starts[0 .. 3 * n_sites] ascends from 0.  EINVAL, nothing written, the message naming the first bad row: read >= n_reads, a
 * cover of 0 or above k, pos or the window beyond the read; also a read table that does not ascend and null pointers.
 * BRISK_HIP_ECAPACITY, nothing written, *n_out_nts (HOST) filled: out_cap_words < ceil(n_nts / 16) + 2.  The output may not overlap
 * the inputs.  Every output word is stored once by a plain vector store.  Needs no index state: works on any handle. */
int brisk_hip_candidate_windows(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                                const brisk_hip_site *d_sites, uint64_t n_sites,
                                uint32_t *d_out_packed, uint64_t out_cap_words, uint64_t *d_out_starts /* 3 * n_sites + 1 room */,
                                uint64_t *n_out_nts /* HOST */);
/* The decisions: d_cand_slots (DEVICE) holds the slots of the candidate stream of d_sites as brisk_hip_get_kmers_packed answers
 * them (3 * cover slots a site, in site order) -> one correction row per corrected site, in site order, d_out_corrections (DEVICE,
 * corr_cap rows of room); `from` is read from the input stream.  Fills n_sites and the three decision counters of *stats (HOST), zero
 * elsewhere.  BRISK_HIP_ECAPACITY when corr_cap < n_corrected: nothing is written, *stats is filled.  EINVAL as for
 * brisk_hip_candidate_windows.  Needs no index state: works on any handle. */
int brisk_hip_decide_sites(brisk_hip_index *h, const uint16_t *d_cand_slots, const brisk_hip_site *d_sites, uint64_t n_sites,
                           const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads, uint32_t solid_min,
                           brisk_hip_correction *d_out_corrections, uint64_t corr_cap, brisk_hip_correct_stats *stats /* HOST */);
/* The patched copy of a packed stream: every word of the input, its two readable words included (out_cap_words >=
 * ceil(d_starts[n_reads] / 16) + 2, else BRISK_HIP_ECAPACITY), with `to` at nucleotide pos of read `read` for every row of
 * d_corr[n_corr] (DEVICE).  EINVAL, nothing written, the message naming the first bad row: read >= n_reads, pos beyond the read, `from`
 * is not the base that is there, to == from or no code, or the table does not strictly ascend by (read, pos); also a read table that
 * does not ascend and null pointers.  The output may not overlap the input.  Every output word is stored once by a plain vector
 * store: the lane that owns a word searches the table, which ascends in absolute nucleotide position.  Works on any handle. */
int brisk_hip_apply_corrections(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                                const brisk_hip_correction *d_corr, uint64_t n_corr, uint32_t *d_out_packed, uint64_t out_cap_words);
/* brisk_hip_get_kmers_packed, weak_sites, candidate_windows, get_kmers_packed over the candidates, decide_sites and
 * apply_corrections in one call, batch by batch like brisk_hip_split_packed.  A batch's slots exist for one internal batch at a time;
 * its sites are decided in rounds of at most BRISK_CORRECT_BATCH sites (environment, read once per process; default 2^22; a test
 * hook), which bounds the scratch memory of a round at roughly 3 * (2 k - 1) / 4 + 6 k bytes a site for the candidate stream and its
 * slots, plus about 128 bytes a site of tables; the correction table accumulates in scratch memory (16 bytes a row, reads numbered as in
 * the call).  Nothing is written to the caller's outputs before the capacities are known to suffice: BRISK_HIP_ECAPACITY when
 * corr_cap < n_corrected (with d_out_corrections != NULL) or out_cap_words < ceil(d_starts[n_reads] / 16) + 2 (with d_out_packed !=
 * NULL), *stats filled.  d_out_corrections may be NULL; d_out_packed == NULL with out_cap_words == 0: the table and the stats only.
 * Inherits brisk_hip_split_packed: pending deferred inserts are completed first; EINVAL on a sharded index, on an entry-id index, on
 * offsets that do not ascend (and on a read of 2^32 nucleotides or more); the answer does not depend on max_batch_reads,
 * BRISK_PROFILE_BATCH, BRISK_PROFILE_SEG, BRISK_CORRECT_BATCH or on which kernels run.  correct_reads takes HOST reads (layout of
 * brisk_hip_get_reads) and returns only the table, out_corrections[corr_cap] HOST, written when it fits: the caller patches its
 * own strings. */
int brisk_hip_correct_packed(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                             uint32_t solid_min, uint32_t min_cover, uint32_t *d_out_packed, uint64_t out_cap_words,
                             brisk_hip_correction *d_out_corrections /* corr_cap room, may be NULL */, uint64_t corr_cap,
                             brisk_hip_correct_stats *stats /* HOST */);
int brisk_hip_correct_reads(brisk_hip_index *h, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                            uint32_t solid_min, uint32_t min_cover, brisk_hip_correction *out_corrections /* HOST */, uint64_t corr_cap,
                            brisk_hip_correct_stats *stats /* HOST */);

/* point lookups of UNHASHED (kmer_s, minimizer_idx) pairs, as Brisk::get takes them.
 * HOST arrays; out_found[i] in {0,1}; out_data[i] valid when found. */
int brisk_hip_lookup(brisk_hip_index *h, const uint64_t *kmer_lo, const uint64_t *kmer_hi, const uint8_t *minimizer_idx,
                     uint64_t n, uint8_t *out_data, uint8_t *out_found);

/* ---- enumeration --------------------------------------------------------- */
/* Walks the index in ascending partition (bucket-range) order, storage order
 * inside one.  *cursor = 0 restarts (restart_kmer_enumeration); the call
 * returns up to cap entries into HOST arrays (k-mers unhashed, as Brisk::next
 * yields them), advances *cursor, and sets *n_out; *n_out == 0 means done. */
int brisk_hip_enumerate(brisk_hip_index *h, uint64_t *cursor, uint64_t *out_lo, uint64_t *out_hi,
                        uint8_t *out_minimizer_idx, uint8_t *out_data, uint64_t cap, uint64_t *n_out);

/* nb_buckets and nb_kmers are exact and order independent; nb_skmers and
 * largest_bucket depend on insertion order in the reference and are reported
 * here as: super-k-mer records received, largest partition (entries). */
int brisk_hip_stats(brisk_hip_index *h, uint64_t *nb_buckets, uint64_t *nb_skmers, uint64_t *nb_kmers,
                    uint64_t *memory_bytes, uint64_t *largest_bucket);

/* Brisk::reallocate (brisk/Brisk.hpp:202-224: the index re-bucketed to (m + 2, b + 2); dormant in the reference): every
 * entry of `from` goes into `to` -- an EMPTY bulk-count index over the same k and device, created by the caller with the
 * new (m, b) and the same count_mode (EINVAL otherwise, the message names count_mode) -- under the identity (kmer_s,
 * minimizer_idx) that SuperKmerEnumerator gives the k-mer at the new m, with its count; entries that the new minimizer maps to
 * one identity merge, counts added mod 256 (saturating indexes: added and clamped to 255).  `from` stays as it is. */
int brisk_hip_reallocate(brisk_hip_index *from, brisk_hip_index *to);

/* Where the arena's memory is (no reference counterpart; Brisk::stats reports the process' peak RSS, brisk/Brisk.hpp:184-189):
 * out[0] = device memory mapped behind this index's arena, out[1] = virtual address range this index has reserved for it
 * (0 without virtual memory management), out[2] = device memory held, process-wide, by the pooled arenas of destroyed
 * indexes (handed to the next index, given back when an allocation fails for lack of memory), out[3] = address space,
 * process-wide, that retired arenas keep reserved for the life of the process (no memory behind it). */
int brisk_hip_memory_info(brisk_hip_index *h, uint64_t out[4]);
/* Entries of arena the single-pass insert sets aside beyond a batch's own need ("every k-mer instance is new"): one partly used
 * private chunk per persistent insert wave (resident waves x chunk entries).  A batch's insert needs room for
 * instances + instances / 7 + this many entries, or it is split in halves (BRISK_HIP_ENOMEM when even one read does not fit). */
int brisk_hip_insert_slack(brisk_hip_index *h, uint64_t *entries);

/* Order-independent digest of the whole index, for parity checks at sizes where the multiset
 * cannot be compared line by line: out[0] = number of entries, out[1] = sum of counts,
 * out[2] = sum over entries of mix(kmer_lo, kmer_hi, minimizer_idx, count) mod 2^64 with
 * mix(a,b,c,d) = f(a ^ f(b ^ f(c << 8 | d))), f = the splitmix64 finaliser (k-mers unhashed,
 * as Brisk::next yields them).  Digests of bucket-range shards add up to the whole index's. */
int brisk_hip_checksum(brisk_hip_index *h, uint64_t out[3]);

/* ---- abundance: spectrum, count-range enumeration, prune (no reference counterpart) ---- */
/* All three compare the STORED count byte: counts are kept mod 256, so an entry whose count wrapped to 0 is an entry with
 * count 0 (it is in bin 0, a range must include 0 to hold it, prune(1, 255) removes it).  All three complete pending
 * deferred inserts first, return EINVAL on an entry-id index (its DATA lives with the caller), and on a sharded handle
 * (n_owners > 1) speak about this owner's partitions only, as brisk_hip_checksum does.  A bound above 255 means 255.
 * In a saturating index (brisk_hip_options.count_mode) no count wraps: bin 0 is empty, bin 255 holds the entries seen 255 times
 * OR MORE, and prune(2, 255) keeps every entry seen at least twice. */
/* out[c] = number of entries whose count is c (HOST array).  Sum over c == nb_kmers of brisk_hip_stats; sum of c * out[c] ==
 * out[1] of brisk_hip_checksum.  Spectra of bucket-range shards add up. */
int brisk_hip_count_spectrum(brisk_hip_index *h, uint64_t out[256]);
/* brisk_hip_enumerate restricted to entries with min_count <= count <= max_count: same cursor protocol, same order (ascending
 * partition, storage order inside one), same outputs.  EINVAL if min_count > max_count.  ECAPACITY only if the PASSING entries
 * of one partition exceed cap.  A walk keeps its bounds from *cursor = 0 to the end. */
int brisk_hip_enumerate_range(brisk_hip_index *h, uint64_t *cursor, uint64_t *out_lo, uint64_t *out_hi,
                              uint8_t *out_minimizer_idx, uint8_t *out_data, uint64_t cap, uint64_t *n_out,
                              uint32_t min_count, uint32_t max_count);
/* Removes, in place, every entry whose count is outside [min_count, max_count]; *removed (may be NULL) receives how many.
 * Afterwards the index is exactly the index that holds the remaining entries: stats (nb_kmers, nb_buckets, largest_bucket),
 * checksum, enumerate, lookup, every get and every later insert behave so (a removed k-mer that is inserted again starts at
 * 1).  Storage order of the survivors is kept.  nb_skmers (records received) is left as it is.  The arena is a bump
 * allocator: a partition's slice keeps its place and capacity, so later inserts fill the room the removed entries left, but
 * no device memory is returned and memory_bytes / brisk_hip_memory_info do not shrink (brisk_hip_clear, or a new index, do
 * that).  EINVAL if min_count > max_count. */
int brisk_hip_prune(brisk_hip_index *h, uint32_t min_count, uint32_t max_count, uint64_t *removed);

/* ---- de Bruijn adjacency: neighbours, degree spectrum, prune by degree (no reference counterpart) ---- */
/* Entry e has the nucleotide string x: the k nucleotides of kmer_s as brisk_hip_enumerate unhashes it, leftmost nucleotide in the
 * highest bits, codes of "ACTG" (0..3).  Its eight neighbour strings, in this order: R_c = x[1:] + c for c = 0..3, then
 * L_c = c + x[:-1] for c = 0..3.  The adjacency byte of e has bit c set when R_c is a neighbour and bit 4 + c when L_c is.  A string
 * is a neighbour when, looked up as a read of exactly k nucleotides -- one brisk_hip_get_kmers slot, under the identity the scan
 * gives that read on its own -- it is present and its stored count byte is >= min_count.  min_count 0 is plain presence (in a
 * wrapping index a present entry with count 0 passes).  Self-loops (homopolymers), palindromes and an entry that is its own
 * reverse complement's neighbour need no rule of their own: the string lookup decides.  "Left" and "right" are relative to the
 * stored orientation of x, which the minimizer's strand chooses, so degree classes are (left, right) pairs and every derived
 * figure is symmetric in them.
 * One canonical k-mer is one entry at k <= 32, and at k > 32 in a full-mode index (brisk_hip_options.minimizer_mode): THE GRAPH
 * WANTS A FULL-MODE INDEX AT k > 32.  In reference mode there a k-mer looked up on its own is not always found (its identity
 * depends on the read around it); the calls are allowed and mean what the lookup means.
 * All three complete pending deferred inserts first, are valid in either count_mode and either minimizer_mode, answer
 * independently of batching, and return EINVAL on an entry-id index and on a sharded handle (n_owners > 1: an entry's neighbours
 * live with other owners; the sharded route is a follow-up). */
/* d_adj (DEVICE, cap bytes): one byte per entry in brisk_hip_enumerate's order -- ascending partition, storage order inside one --
 * so row i of a full enumeration and d_adj[i] are the same entry.  *n_entries receives nb_kmers.  ECAPACITY, with nothing
 * written, when cap < nb_kmers. */
int brisk_hip_adjacency(brisk_hip_index *h, uint32_t min_count, uint8_t *d_adj, uint64_t cap, uint64_t *n_entries);
/* out (HOST): the nodes are the entries whose own count is >= min_count; out[5 * left + right] counts the nodes with `left` set
 * bits among bits 4..7 of their byte and `right` among bits 0..3; out[25] counts the entries below min_count (not nodes).
 * The 26 values always sum to nb_kmers of brisk_hip_stats. */
int brisk_hip_degree_spectrum(brisk_hip_index *h, uint32_t min_count, uint64_t out[26]);
/* Removes, in place, every node (count >= min_count) whose count is <= max_count and whose class bit 1u << (5 * left + right) is
 * set in class_mask; *removed (may be NULL) receives how many.  Adjacency is taken once, over the index as it stands when the
 * call begins, and is not iterated: two dead ends that touch each other are both judged by the graph before the call.  Entries
 * below min_count are never removed here (that is brisk_hip_prune's job).  Afterwards everything brisk_hip_prune promises
 * holds: storage order of the survivors, stats including nb_buckets, checksum, lookups, later inserts (a removed k-mer starts
 * at 1 again), no memory returned.  EINVAL if min_count > max_count or class_mask has a bit above 24. */
int brisk_hip_prune_degrees(brisk_hip_index *h, uint32_t min_count, uint32_t max_count, uint32_t class_mask, uint64_t *removed);
/* Device time in ms of the last of the three calls above, while brisk_hip_profile_enable is on (zeros otherwise):
 * out[0] the neighbour-read kernel, out[1] the lookups, out[2] the fold (and the histogram), summed over the call's rounds. */
int brisk_hip_graph_phase_ms(brisk_hip_index *h, double out[3]);

/* ---- set operations: merge, intersect, subtract, compare (no reference counterpart) ---- */
/* Two indexes created with the same (k, m, b) and the same partition layout route an identity to the same partition and store it
 * as the same key bits, so they are combined on the device partition by partition, keys compared as stored.
 * Identity is (kmer_s, minimizer_idx), as everywhere else.  Presence is what counts: an entry whose stored count wrapped to 0 is
 * present with count 0.  `src` (and both sides of compare) is left bit for bit as it was: same checksum, same enumeration order.
 * Both handles must agree in k, m, b, part_bits, ext_bits, cls_bits, cls_width, count_mode (brisk_hip_layout) and key width, and
 * live on the same device: otherwise BRISK_HIP_EINVAL, with a message (brisk_hip_last_error of the first handle) that names the field that
 * differs.  EINVAL also for a null handle, dst == src, an entry-id index or a sharded handle (n_owners > 1) on either side, and
 * an unknown count_rule; nothing is changed then.  The counter pointers may be NULL.  Pending deferred inserts of BOTH handles
 * are completed first; both per-handle locks are held for the call (taken together, as brisk_hip_reallocate takes them), and
 * src's stream is synchronised before dst's stream reads src's arena. */
enum { BRISK_HIP_COUNT_LEFT = 0, BRISK_HIP_COUNT_MIN = 1, BRISK_HIP_COUNT_MAX = 2, BRISK_HIP_COUNT_SUM = 3 };
/* dst := dst UNION src; the count of a shared entry is dst + src mod 256 (saturating indexes: min(255, dst + src)); *added = entries new to dst.  Afterwards dst is exactly
 * the index that inserting src's reads after dst's reads would have given: the same multiset of (kmer, minimizer_idx, count), so
 * the same checksum, nb_kmers and nb_buckets; nb_skmers becomes dst's plus src's.  Entries already in dst keep their storage
 * order; where new ones land is not specified.  BRISK_HIP_ENOMEM as for an insert (src's entries go through dst's insert as
 * one-k-mer records that carry their counts). */
int brisk_hip_merge(brisk_hip_index *dst, brisk_hip_index *src, uint64_t *added);
/* dst keeps the entries whose identity is also in src; their count follows count_rule: LEFT dst's, MIN / MAX of the two,
 * SUM dst + src mod 256 (saturating indexes: min(255, dst + src)).  *removed = entries dst lost.
 * After intersect and subtract dst is exactly the index that holds the remaining entries, as after brisk_hip_prune: stats
 * (nb_kmers, nb_buckets, largest_bucket), checksum, enumerate, lookup, every get and every later insert behave so.  Survivors
 * keep their storage order.  A partition's slice keeps its offset and capacity and no device memory is returned; nb_skmers is
 * left as it is. */
int brisk_hip_intersect(brisk_hip_index *dst, brisk_hip_index *src, uint32_t count_rule, uint64_t *removed);
/* dst loses the entries whose identity is in src, whatever the counts */
int brisk_hip_subtract(brisk_hip_index *dst, brisk_hip_index *src, uint64_t *removed);
/* read-only. out[0] entries in both, out[1] only in a, out[2] only in b,
 * out[3] sum over shared of min(count_a, count_b), out[4] sum of count_a over shared, out[5] sum of count_b over shared */
int brisk_hip_compare(brisk_hip_index *a, brisk_hip_index *b, uint64_t out[6]);

/* ---- the joint count spectrum and the joint count-window filter ---- */
/* Two more set operations: the same compatibility fields and messages, the same refusals (a null handle, dst == src, an
 * entry-id index or a sharded handle on either side, a count_mode mismatch: EINVAL), the same two locks, pending deferred
 * inserts of both handles completed first, src's stream synchronised before it is read.  Both compare STORED count bytes. */
#define BRISK_HIP_JOINT_ABSENT 256u
#define BRISK_HIP_JOINT_STATES 257u
/* read-only. out is a HOST array of 257*257 uint64. out[sa*257 + sb] = number of identities whose state in a is sa and in b
 * is sb. A state is the STORED count byte (0..255) of a present entry, or 256 = not in that index. A wrapped count of 0 is
 * present with state 0, never state 256. out[256*257+256] = 0.  EINVAL if out is NULL.
 * Both indexes are left bit for bit as they were.  Between saturating indexes bin 255 means "255 or more" on either axis and
 * state 0 is never populated.  By construction: rows 0..255 sum to a's brisk_hip_count_spectrum and columns 0..255 to b's; the
 * present x present block sums to brisk_hip_compare's out[0], and weighted by sa, by sb and by min(sa, sb) to its out[4],
 * out[5] and out[3]; row 256 sums to its out[2], column 256 to its out[1]. */
int brisk_hip_joint_spectrum(brisk_hip_index *a, brisk_hip_index *b, uint64_t *out);

typedef struct brisk_hip_joint_window {
    uint32_t min_self, max_self;    /* dst's stored count must lie in [min_self, max_self]; a bound above 255 means 255 */
    uint32_t min_other, max_other;  /* an entry whose identity IS in src passes if src's stored count lies in this range;
                                       min_other > max_other: no entry that is present in src passes */
    uint32_t keep_absent;           /* non-zero: an entry whose identity is NOT in src passes the src side */
    uint32_t reserved;              /* must be 0 */
} brisk_hip_joint_window;
/* dst keeps the entries that pass both sides, with their counts unchanged; *removed (may be NULL) = entries dst lost.
 * Afterwards dst is exactly the index that holds the remaining entries, as after brisk_hip_intersect or brisk_hip_prune
 * (stats, checksum, enumerate, lookup, every get, every later insert; survivors keep their storage order, slices their offset
 * and capacity, nb_skmers stays); src is left bit for bit as it was.  EINVAL, checked before any device call, nothing changed
 * and *removed not written: w is NULL, min_self > max_self, reserved != 0, or a window nothing can pass (min_other > max_other
 * with keep_absent == 0).  In a saturating index a bound of 255 keeps everything seen at least 255 times.
 * By construction: {0,255, 0,255, 0} is intersect(LEFT); {0,255, 1,0, 1} is subtract; {lo,hi, 0,255, 1} is prune(lo, hi). */
int brisk_hip_filter_joint(brisk_hip_index *dst, brisk_hip_index *src, const brisk_hip_joint_window *w, uint64_t *removed);

/* ---- snapshots: an index saved to a file and loaded back (no reference counterpart) ---- */
/* An entry's stored key plus its partition number is its whole identity, so a snapshot is the directory and the live entries of
 * every slice, as stored: nothing is unhashed, scanned or inserted again.  The file format (version 1, little-endian: a 256-byte
 * header, then blocks of whole partitions in ascending order) is specified byte by byte in DESIGN.md section 4.w.
 * All three: EINVAL on a null handle or path.  save and load: EINVAL on an entry-id index and on a sharded handle (n_owners > 1);
 * pending deferred inserts are completed first; the handle's lock is held for the call; the file streams through two pinned host
 * buffers of one block each (device <-> host of one block runs under the file I/O of its neighbour), so host memory does not grow
 * with the index.  BRISK_HIP_EIO: the file system refused; BRISK_HIP_EFORMAT: the bytes are not a consistent version-1 snapshot. */
enum { BRISK_HIP_LOAD_COMPACT = 0, BRISK_HIP_LOAD_ROOM = 1 };
typedef struct brisk_hip_snapshot_info {
    uint32_t struct_size;       /* sizeof(brisk_hip_snapshot_info), set by the caller */
    uint32_t version, header_bytes;
    uint32_t k, m, b, data_bytes;
    uint32_t part_bits, ext_bits, cls_bits, cls_width; /* as brisk_hip_layout */
    uint32_t key_words;         /* u64 words per stored key: 1 or 2 */
    uint32_t shift;             /* 2b + ext_bits - part_bits: routing-id bits kept inside a key */
    uint32_t minimizer_mode;    /* brisk_hip_options.minimizer_mode of the saved index (header offset 116; 0 in files written before
                                 * the field existed: the reference's minimizers).  It lies in what was padding before n_entries: no
                                 * other member moved */
    uint64_t n_entries, n_partitions /* non-empty ones */, nb_skmers;
    uint64_t checksum[3];       /* brisk_hip_checksum at save time */
    uint64_t n_blocks;
    uint64_t file_bytes;        /* length of the file (not stored in it) */
    uint32_t count_mode;        /* brisk_hip_options.count_mode of the saved index (header offset 112; 0 in files written before
                                 * the field existed: counts wrap).  A caller whose struct_size ends before it sees no change */
} brisk_hip_snapshot_info;
/* The header of a snapshot file.  Host only: no device and no handle are needed.  EIO: the file cannot be opened or is shorter than
 * a header; EFORMAT: wrong magic, a version other than 1, an unknown count_mode or minimizer_mode, or sizes that disagree with the file's length (brisk_hip_load
 * answers EIO for a file that is shorter than its header says: it ends early). */
int brisk_hip_snapshot_info_read(const char *path, brisk_hip_snapshot_info *out);
/* Writes the index to `path`; *entries_written (may be NULL) receives the entries.  The bytes go to `path` plus a temporary suffix
 * and are renamed at the end: a file under the final name is always whole, and a failed save leaves none behind.  Live entries
 * only: the room a prune or subtract left inside slices, and abandoned slices, are not written.  The index is left bit for bit as
 * it was (same checksum, same enumeration order), and two saves of one index are the same bytes.  The writer cuts blocks of about
 * 2^24 entries; the environment variable BRISK_SNAPSHOT_BLOCK=<entries>, read at each call, sets another limit (a test hook). */
int brisk_hip_save(brisk_hip_index *h, const char *path, uint64_t *entries_written);
/* Reads a snapshot into an EMPTY bulk-count index (EINVAL otherwise: "load into an empty index, or load into a second handle and
 * merge") whose k, m, b, data_bytes, part_bits, ext_bits, cls_bits, cls_width, key_words, shift, count_mode and minimizer_mode are the file's (EINVAL otherwise;
 * the message names the first field that differs).  Afterwards the handle is what it would be had it inserted the entries: every
 * call behaves so, enumeration order is the saved index's, nb_skmers is the saved one.  flags: BRISK_HIP_LOAD_COMPACT -- every slice
 * exactly as large as its entries, slices back to back: the file's bytes go straight into the arena, and this is the compaction
 * that brisk_hip_prune cannot do; BRISK_HIP_LOAD_ROOM -- every slice with the room an insert would have given it, for an index that
 * keeps growing (an insert into a compact slice moves it).  When the last block is in, the digest of the loaded index is compared
 * with the header's (EFORMAT on a mismatch).  BRISK_HIP_ENOMEM as for an insert (BRISK_ARENA_LIMIT is honoured).  After any failed
 * load the handle is the empty index and usable.  *entries_read may be NULL. */
int brisk_hip_load(brisk_hip_index *h, const char *path, uint32_t flags, uint64_t *entries_read);

/* ---- the path cut at the super-k-mer boundary (multi-GPU) ----------------- */
/* scan: d_records receives up to cap_records records of record_words u64 each;
 * *n_records (HOST) receives the count.  BRISK_HIP_ECAPACITY if cap is too small
 * (nothing is inserted by a scan, so the call can simply be repeated). */
int brisk_hip_scan_packed(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                          uint64_t *d_records, uint64_t cap_records, uint64_t *n_records);
/* upper bound on the records a scan of these reads can emit (HOST result) */
int brisk_hip_scan_bound(brisk_hip_index *h, const uint64_t *d_starts, uint64_t n_reads, uint64_t *bound);
/* route: reorder records so that each owner's records are contiguous, owner 0
 * first; counts[n_owners] (HOST) receives records per owner.  d_out may not alias d_in. */
int brisk_hip_route_records(brisk_hip_index *h, const uint64_t *d_records, uint64_t n_records,
                            uint64_t *d_out, uint64_t *counts);
/* insert records whose buckets this index owns */
int brisk_hip_insert_records(brisk_hip_index *h, const uint64_t *d_records, uint64_t n_records);
/* The scan of a sharded index also counts its records per bucket-range partition (records in the low,
 * k-mer instances in the high 32 bits).  export_hist copies that histogram (2^part_bits u64, partition
 * order = owner order) to d_hist_out right after brisk_hip_scan_packed; partitions_per_owner[n_owners]
 * (HOST) receives the length of each owner's slice, so that the slices can travel with the records.
 * insert_records_hist is insert_records for an owner that received one such slice of ITS range from
 * each scanning rank (n_slices slices of equal length, back to back): it adds them up instead of
 * counting the received records again.  export_hist_add ADDS the histogram to d_hist_acc (2^part_bits u64 the
 * caller zeroed) instead: a rank that scans its reads in several pieces sends one summed slice per owner per
 * batch, not one per piece. */
int brisk_hip_export_hist(brisk_hip_index *h, uint64_t *d_hist_out, uint64_t *partitions_per_owner);
int brisk_hip_export_hist_add(brisk_hip_index *h, uint64_t *d_hist_acc, uint64_t *partitions_per_owner);
int brisk_hip_insert_records_hist(brisk_hip_index *h, const uint64_t *d_records, uint64_t n_records,
                                  const uint64_t *d_hist_slices, uint32_t n_slices);
/* Ownership of a sharded index (n_owners > 1): owner o holds the contiguous partition range [first_partition[o],
 * first_partition[o + 1]) (HOST array of n_owners + 1 entries, first_partition[0] = 0, first_partition[n_owners] = 2^part_bits,
 * ascending; an owner may hold nothing).  By default the ranges are equal (owner = partition * N >> part_bits).  Equal ranges do
 * not carry equal loads -- a partition is a range of minimizer-hash values and minimizers are the smallest hashes of their
 * windows ("histogram-balanced cut points if skew > 1.3x") -- so a job takes its cut points from the
 * partition histogram of a first scan (export_hist, all ranks' histograms added up) and hands the SAME array to every rank
 * before anything is routed or inserted: EINVAL on an index that holds entries.  No reference counterpart (single process). */
int brisk_hip_set_owner_cuts(brisk_hip_index *h, const uint64_t *first_partition);
/* The query path cut at the same boundary.  scan_query = the scan as query_sequence runs it (a read's
 * enumeration stops at the first super-k-mer after the first whose returned minimizer is 0,
 * apps/counter.cpp:304-306); d_tags[i] = index of the read record i came from.  route_tagged = route_records
 * carrying the tags along.  query_records: d_sums[i] = sum of the counts of record i's k-mers present in
 * THIS index (records whose buckets it owns), what Brisk::get_superkmer + the caller's loop add up
 * (brisk/Brisk.hpp:102-118, apps/counter.cpp:296-303).  A sharded get is scan_query -> route_tagged ->
 * all-to-all -> query_records on the owner -> all-to-all back -> per_read[tag] += sum.
 * With BRISK_HIP_ECAPACITY, *n_records is an upper bound only: long sequences are scanned in chunks, and the records
 * of chunks that are cut or scanned again are counted before they are dropped (brisk_hip_scan_bound always suffices). */
int brisk_hip_scan_query(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                         uint64_t *d_records, uint32_t *d_tags, uint64_t cap_records, uint64_t *n_records);
int brisk_hip_route_tagged(brisk_hip_index *h, const uint64_t *d_records, const uint32_t *d_tags, uint64_t n_records,
                           uint64_t *d_out, uint32_t *d_tags_out, uint64_t *counts);
int brisk_hip_query_records(brisk_hip_index *h, const uint64_t *d_records, uint64_t n_records, uint64_t *d_sums);

/* The per-k-mer get (brisk_hip_get_kmers) cut at the same boundary.  The owner of a bucket range does not hold the asker's slot array,
 * so it answers into a compact buffer that travels back: record i's k-mers, in the record's own order (the order its key is built
 * in: minimizer_idx rising), at offsets[i] .. offsets[i + 1], offsets being the exclusive prefix sum of the records' k-mer counts.
 * Asker and owner compute the same table from the records alone (record_kmers), so only records travel out and only answers travel
 * back -- no tags, no anchors: the asker keeps those and turns position-in-record into position-in-read itself.  A sharded
 * per-k-mer get is scan_kmers -> route_tagged -> all-to-all -> record_kmers + answer_records on the owner -> all-to-all back (u16,
 * split sizes = the differences of the asker's table at the owner boundaries) -> record_kmers + place_answers.  All five take the
 * per-handle lock, run on the handle's stream, complete pending deferred inserts first and return when their output is complete. */
/* The scan of brisk_hip_get_kmers_packed (every k-mer: no query stop at a returned minimizer of 0), cut at the record boundary as
 * brisk_hip_scan_query is.  Per record i: the record, d_tags[i] = an index into d_anchors (route_tagged carries it along) and the
 * record's slot anchor there (opaque: a slot of the batch's slot array, layout of brisk_hip_get_kmers_packed, plus an orientation
 * bit).  *n_slots (HOST, 64-bit) = the batch's slots.  d_records, d_tags, d_anchors hold cap_records entries each; ECAPACITY and
 * brisk_hip_scan_bound as for brisk_hip_scan_query.  Sequences of more than 8192 k-mers are scanned in chunks, as everywhere.
 * Needs no index state: any handle serves, sharded ones included (the records' routing ids are the handle's layout's). */
int brisk_hip_scan_kmers(brisk_hip_index *h, const uint32_t *d_packed, const uint64_t *d_starts, uint64_t n_reads,
                         uint64_t *d_records, uint32_t *d_tags, uint64_t *d_anchors, uint64_t cap_records,
                         uint64_t *n_records, uint64_t *n_slots);
/* d_offsets[0 .. n_records] (DEVICE, u64) = the exclusive prefix sum of the records' k-mer counts; d_offsets[n_records] = their total.
 * For records grouped by owner (route_tagged) the answers owed by owner o are the difference of the table at o's group boundaries.
 * Any handle of the records' geometry.  At most 2^32 - 1 records. */
int brisk_hip_record_kmers(brisk_hip_index *h, const uint64_t *d_records, uint64_t n_records, uint64_t *d_offsets);
/* Owner side.  d_answers[d_offsets[i] + j] (DEVICE, u16, d_offsets[n_records] entries; d_offsets from record_kmers over the same
 * records) = 0 when k-mer j of record i is absent from THIS index, 0x100 | count when present -- the slot values of
 * brisk_hip_get_kmers.  Every one of the d_offsets[n_records] entries is written and nothing else is.  Records of other owners, the
 * limit of 2^32 - 1 records and pending inserts: as for brisk_hip_query_records.  The probe kernels are those of
 * brisk_hip_get_kmers (same selection, same environment switches), run under anchors made from d_offsets.  EINVAL on an entry-id index. */
int brisk_hip_answer_records(brisk_hip_index *h, const uint64_t *d_records, uint64_t n_records, const uint64_t *d_offsets,
                             uint16_t *d_answers);
/* Asker side.  For the routed records (d_records, d_tags as route_tagged left them, or any contiguous piece of them with its own
 * record_kmers table and the answers that came back for it) and the anchors of the scan_kmers call they come from:
 * d_slots[slot of k-mer j of record i] = d_answers[d_offsets[i] + j], by plain vector stores.  Every slot of the batch belongs to
 * exactly one k-mer of one record, so when every piece has been placed every slot has been written once; several calls may fill
 * one slot array.  A slot >= n_slots is never stored: the call then returns EINVAL (a broken anchor: not the anchors of these
 * records, or n_slots too small), the slots below n_slots hold what was placed, and the handle stays usable.  Any handle of the
 * records' geometry. */
int brisk_hip_place_answers(brisk_hip_index *h, const uint64_t *d_records, const uint32_t *d_tags, const uint64_t *d_anchors,
                            uint64_t n_records, const uint64_t *d_offsets, const uint16_t *d_answers,
                            uint16_t *d_slots, uint64_t n_slots);
/* The reduction of brisk_hip_read_profile_packed over slots the caller holds (DEVICE; layout of brisk_hip_get_kmers_packed for the
 * reads d_starts[0 .. n_reads] describes): d_out[r] = the record of read r.  Same records, same BRISK_PROFILE_SEG segment rule, same
 * refusals (offsets that do not ascend, a read of more than 2^32 - 1 slots).  Needs no index state: any handle serves. */
int brisk_hip_profile_slots(brisk_hip_index *h, const uint16_t *d_slots, const uint64_t *d_starts, uint64_t n_reads,
                            uint32_t solid_min, brisk_hip_read_profile *d_out);

/* ---- the per-call API under the C++ facade (entry-id mode) --------------------- */
/* SuperKmerEnumerator over one clean sequence (len >= k): every vector next() would
 * return, in order.  HOST arrays: skm_ret/skm_n sized >= len-k+1 vectors, km_* sized
 * >= cap_kmers >= len-k+1 k-mers (k-mers unhashed, vector after vector). */
int brisk_hip_scan_sequence(brisk_hip_index *h, const char *bases, uint64_t len, uint64_t cap_kmers,
                            uint64_t *skm_ret, uint32_t *skm_n, uint64_t *km_lo, uint64_t *km_hi, uint8_t *km_idx,
                            uint64_t *n_skm);
/* insert_superkmer: find-all then insert-missing for the k-mers of one vector, in order.
 * ids[i] = the entry's dense id, newly[i] = 1 if this call created it (its DATA is then
 * uninitialised, as in the reference).  HOST arrays; n <= 255. */
int brisk_hip_upsert_kmers(brisk_hip_index *h, const uint64_t *kmer_lo, const uint64_t *kmer_hi, const uint8_t *minimizer_idx,
                           uint64_t n, uint32_t *ids, uint8_t *newly);
/* get_superkmer / get: ids[i] = entry id or 0xffffffff when absent */
int brisk_hip_find_kmers(brisk_hip_index *h, const uint64_t *kmer_lo, const uint64_t *kmer_hi, const uint8_t *minimizer_idx,
                         uint64_t n, uint32_t *ids);
/* next(): as brisk_hip_enumerate, returning entry ids instead of counts */
int brisk_hip_enumerate_ids(brisk_hip_index *h, uint64_t *cursor, uint64_t *out_lo, uint64_t *out_hi,
                            uint8_t *out_minimizer_idx, uint32_t *out_ids, uint64_t cap, uint64_t *n_out);

/* ---- helpers on device buffers -------------------------------------------- */
int brisk_hip_pack_ascii(brisk_hip_index *h, const char *d_bases, uint64_t n_bases, uint32_t *d_packed);
/* the inverse: d_bases[i] = "ACTG"[code of nucleotide first_nt + i of the packed stream], i < n_nts (upper case; DEVICE buffers).
 * Words past the one that holds nucleotide first_nt + n_nts - 1 are not read.  Queued on the handle's stream, as pack_ascii is. */
int brisk_hip_unpack_ascii(brisk_hip_index *h, const uint32_t *d_packed, uint64_t first_nt, uint64_t n_nts, char *d_bases);
/* synthetic reads of SURVEY.md 8(d), written packed; d_starts[n_reads+1] */
int brisk_hip_synth_reads(brisk_hip_index *h, uint64_t genome_len, uint64_t first_read, uint64_t n_reads,
                          uint32_t read_len, uint64_t seed_g, uint64_t seed_r,
                          uint32_t *d_packed, uint64_t *d_starts);

/* ---- test hooks -------------------------------------------------------------- */
/* order keys (bfc_hash_64, brisk/hashing.cpp:8-19) of n m-mers, computed by the device
 * code path the scan uses (table-driven class with guard band when exact == 0, the
 * plain FP64 fold when exact != 0).  HOST arrays. */
int brisk_hip_debug_order_keys(brisk_hip_index *h, const uint64_t *mmers, uint64_t n, int exact, uint64_t *keys);
/* The fast path runs the body the scan of the handle's geometry runs: where (k, m) has a scan with k and m as compile-time
 * constants (63,21; 31,15; 31,11) that body's order key, else the run-time layout with the scan's chunk-count unrolling.
 * brisk_hip_debug_guard_count: how many keys of the handle's LAST brisk_hip_debug_order_keys call had a class sum inside the
 * guard band and were decided by the exact FP64 fold (0 after an exact != 0 call; all of them in a -DCLS_FORCE_GUARD build). */
int brisk_hip_debug_guard_count(brisk_hip_index *h, uint64_t *n_guard);
/* brisk_hip_debug_touched: the partitions the handle's LAST record insert touched, in the order its insert kernels walked them
 * (ascending inside a block of 8192 partitions; the blocks in the order the device took them, which is not the same from run to
 * run).  *n: their number; the first min(cap, *n) go to parts.  Valid until the handle's next insert or query.  HOST arrays. */
int brisk_hip_debug_touched(brisk_hip_index *h, uint32_t *parts, uint64_t cap, uint64_t *n);
/* brisk_hip_debug_directory: entries in use and slice capacity of n partitions.  HOST arrays. */
int brisk_hip_debug_directory(brisk_hip_index *h, const uint32_t *parts, uint64_t n, uint32_t *cnt, uint32_t *cap);

/* ---- measurement ----------------------------------------------------------- */
/* With profiling on, every kernel launch is bracketed by HIP events on the
 * handle's stream.  brisk_hip_profile_read returns, per kernel slot, launches
 * and total milliseconds since the last reset. */
#define BRISK_HIP_PROFILE_SLOTS 16
int brisk_hip_profile_enable(brisk_hip_index *h, int on);
int brisk_hip_profile_read(brisk_hip_index *h, uint32_t *n_slots, const char **names, uint64_t *launches, double *ms);
int brisk_hip_profile_reset(brisk_hip_index *h);

#ifdef __cplusplus
}
#endif
#endif /* BRISK_HIP_H */
