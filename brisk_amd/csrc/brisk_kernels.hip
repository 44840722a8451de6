// brisk_kernels.hip -- HIP kernels of the Brisk hot path for gfx950 (MI355X).
//
// One translation unit, thirteen parts:
//   brisk_scan.hip       reads -> super-k-mer records (SuperKmerEnumerator::next, Kmers.cpp:522-603,
//                        + hash_kmer_minimizer_inplace / get_compacted, Kmers.cpp:138-145,191-200); long sequences in chunks
//   brisk_partition.hip  records -> partition order (histogram prefix, k_scatter) and -> owner order (multi-GPU routing)
//   brisk_insert.hip     per partition: find-all, insert-missing, count++  (DenseMenuYo.hpp:248-310, counter.cpp:262-269)
//   brisk_readout.hip    Brisk::get / get_superkmer / next / stats and the per-call upsert of the facade
//   brisk_answers.hip    the per-position get across bucket-range shards: answer offsets, synthetic anchors, answers -> slots
//   brisk_setops.hip     two indexes combined partition by partition: intersect / subtract / compare, entries -> records for merge
//   brisk_snapshot.hip   the live entries of a partition range to and from a dense buffer: save / load of an index file
//   brisk_profile.hip    the per-position answers of a batch reduced to one abundance record per read
//   brisk_extract.hip    records -> nucleotide intervals, and the kept intervals of a packed stream gathered into a new one
//   brisk_intake.hip     raw bytes and qualities -> fragments (maximal clean runs of a read), gathered into a packed stream
//   brisk_split.hip      slots -> the solid runs of every read as fragments (over the intake's passes), a fragment table -> the gather's tables
//   brisk_correct.hip    slots -> the weak runs that one substitution explains (sites), their candidate windows, the decisions, the patched stream
//   brisk_pairs.hip      paired-end bookkeeping over intervals: one interval per raw read, the pair decision, two cuts chained, pairs / singles split
//
// All of it is integer / byte work (plus the FP64 decycling class); there is no MFMA-shaped work on this path.
#include "brisk_device.h"

#define SCAN_BLOCK 256
#define EMPTY_SLOT 0xffffffffu
#define MATCHED_BIT 0x80000000u

#include "brisk_scan.hip"
#include "brisk_partition.hip"
#include "brisk_insert.hip"
#include "brisk_readout.hip"
#include "brisk_answers.hip"
#include "brisk_setops.hip"
#include "brisk_snapshot.hip"
#include "brisk_profile.hip"
#include "brisk_extract.hip"
#include "brisk_intake.hip"
#include "brisk_split.hip"
#include "brisk_correct.hip"
#include "brisk_pairs.hip"
