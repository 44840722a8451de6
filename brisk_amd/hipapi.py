"""ctypes binding of include/brisk_hip.h (one-to-one; no logic)."""
from __future__ import annotations

import atexit
import ctypes as C
import math
import os
import subprocess
import sys
import weakref
from typing import Optional, Sequence, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB_NAME = os.environ.get("BRISK_HIP_LIB", "libbrisk_hip.so")

STATUS = {0: "OK", 1: "EINVAL", 2: "EUNSUPPORTED", 3: "EHIP", 4: "ENOMEM", 5: "ECAPACITY", 6: "ENODEVICE", 7: "EIO", 8: "EFORMAT"}
ECAPACITY = 5


class BriskHipError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        self.code = code
        super().__init__(f"brisk_hip: {STATUS.get(code, code)} {msg}".strip())


def library_path() -> str:
    return os.path.join(HERE, _LIB_NAME)


def build_library(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU). In-tree output."""
    out = library_path()
    csrc = os.path.join(HERE, "csrc")  # one translation unit, brisk_capi.hip, which includes every other part: all of them make the library stale
    srcs = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(ROOT, "include", "brisk_hip.h"))
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs):
        return out
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread", "-fvisibility=hidden",
           "-Wno-unused-value", "-o", out, os.path.join(csrc, "brisk_capi.hip")]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def build_apps(verbose: bool = False) -> dict:
    """C++ host side: this repo's brisk_count and brisk_shard over the facade headers.  (The reference's own
    apps/counter.cpp, compiled UNCHANGED against brisk_amd/include, is test infrastructure: oracle/Makefile.)"""
    apps = os.path.join(HERE, "apps")
    inc = ["-I" + os.path.join(HERE, "include"), "-I" + os.path.join(ROOT, "include")]
    link = ["-L" + HERE, "-lbrisk_hip", "-Wl,-rpath,$ORIGIN/.."]
    out = {}
    cmd = ["g++", "-std=gnu++17", "-O2", "-pthread"] + inc + [os.path.join(apps, "brisk_count.cpp")] + link + ["-lz", "-o", os.path.join(apps, "brisk_count")]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    out["brisk_count"] = os.path.join(apps, "brisk_count")
    # the multi-GPU job from C++: one process per GPU, RCCL grouped send/recv (apps/brisk_shard.cpp)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=gnu++17", "-O2", "-pthread", "-D__HIP_PLATFORM_AMD__"] + inc + ["-I" + os.path.join(rocm, "include"), os.path.join(apps, "brisk_shard.cpp")] + link + \
          ["-L" + os.path.join(rocm, "lib"), "-lrccl", "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", os.path.join(apps, "brisk_shard")]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    out["brisk_shard"] = os.path.join(apps, "brisk_shard")
    return out


def coef_table(m: int) -> np.ndarray:
    """DecyclingSet(m) coefficients (reference brisk/Decycling.cpp:7-13), computed on
    the HOST with libm; the device only ever sees these bits."""
    unit = 2 * math.pi / m
    coef = np.zeros(4 * m, dtype=np.float64)
    for j in range(1, m):
        s = math.sin(unit * float(j))
        coef[4 * j + 1] = s
        coef[4 * j + 2] = 2 * s
        coef[4 * j + 3] = 3 * s
    return coef


class _Options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("stream", C.c_void_p), ("part_bits", C.c_uint32),
                ("owner_rank", C.c_uint32), ("n_owners", C.c_uint32), ("minimizer_mode", C.c_uint32), ("arena_entries", C.c_uint64),
                ("max_batch_reads", C.c_uint64), ("entry_ids", C.c_uint32), ("immediate_inserts", C.c_uint32),
                ("count_mode", C.c_uint32)]


# brisk_hip_options.count_mode: BRISK_HIP_COUNTS_WRAP / BRISK_HIP_COUNTS_SATURATE
COUNT_MODES = {"wrap": 0, "saturate": 1}
# brisk_hip_options.minimizer_mode: BRISK_HIP_MINIMIZER_REFERENCE / BRISK_HIP_MINIMIZER_FULL
MINIMIZER_MODES = {"reference": 0, "full": 1}


class _Layout(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("k", "m", "b", "m_reduc", "compacted_size", "allocated_bytes", "record_words",
                                          "part_bits", "n_owners", "owner_rank", "ext_bits", "cls_bits", "cls_width", "count_mode")]


class _SnapshotInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "version", "header_bytes", "k", "m", "b", "data_bytes", "part_bits", "ext_bits", "cls_bits",
                                          "cls_width", "key_words", "shift", "minimizer_mode")] + \
               [(n, C.c_uint64) for n in ("n_entries", "n_partitions", "nb_skmers")] + [("checksum", C.c_uint64 * 3), ("n_blocks", C.c_uint64), ("file_bytes", C.c_uint64), ("count_mode", C.c_uint32)]


class _JointWindow(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("min_self", "max_self", "min_other", "max_other", "keep_absent", "reserved")]


# brisk_hip_joint_spectrum: the state "not in that index", and the edge of the matrix
JOINT_ABSENT = 256
JOINT_STATES = 257

_u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")

# every symbol include/brisk_hip.h declares
SYMBOLS = [
    "brisk_hip_abi_version", "brisk_hip_create", "brisk_hip_destroy", "brisk_hip_clear", "brisk_hip_last_error", "brisk_hip_sync",
    "brisk_hip_get_layout", "brisk_hip_get_minimizer_mode", "brisk_hip_insert_reads", "brisk_hip_insert_packed", "brisk_hip_get_reads", "brisk_hip_lookup",
    "brisk_hip_enumerate", "brisk_hip_stats", "brisk_hip_memory_info", "brisk_hip_insert_slack", "brisk_hip_reallocate", "brisk_hip_checksum", "brisk_hip_scan_packed", "brisk_hip_scan_bound", "brisk_hip_route_records",
    "brisk_hip_get_packed", "brisk_hip_get_kmers", "brisk_hip_get_kmers_packed", "brisk_hip_insert_records", "brisk_hip_set_owner_cuts", "brisk_hip_export_hist", "brisk_hip_export_hist_add", "brisk_hip_insert_records_hist", "brisk_hip_scan_query", "brisk_hip_route_tagged", "brisk_hip_query_records", "brisk_hip_pack_ascii", "brisk_hip_synth_reads", "brisk_hip_debug_order_keys", "brisk_hip_debug_guard_count", "brisk_hip_debug_touched", "brisk_hip_debug_directory", "brisk_hip_scan_sequence", "brisk_hip_upsert_kmers", "brisk_hip_find_kmers",
    "brisk_hip_enumerate_ids", "brisk_hip_count_spectrum", "brisk_hip_enumerate_range", "brisk_hip_prune",
    "brisk_hip_read_profile_reads", "brisk_hip_read_profile_packed",
    "brisk_hip_scan_kmers", "brisk_hip_record_kmers", "brisk_hip_answer_records", "brisk_hip_place_answers", "brisk_hip_profile_slots",
    "brisk_hip_select_intervals", "brisk_hip_extract_packed", "brisk_hip_trim_packed", "brisk_hip_trim_reads", "brisk_hip_unpack_ascii",
    "brisk_hip_intake_ascii", "brisk_hip_intake_reads", "brisk_hip_insert_raw_reads",
    "brisk_hip_fragment_intervals", "brisk_hip_pair_intervals", "brisk_hip_compose_intervals", "brisk_hip_extract_pairs_packed",
    "brisk_hip_trim_pairs_packed", "brisk_hip_trim_pairs_reads", "brisk_hip_clean_pairs_ascii", "brisk_hip_clean_pairs_reads",
    "brisk_hip_solid_runs", "brisk_hip_extract_fragments_packed", "brisk_hip_split_packed", "brisk_hip_split_reads",
    "brisk_hip_weak_sites", "brisk_hip_candidate_windows", "brisk_hip_decide_sites", "brisk_hip_apply_corrections", "brisk_hip_correct_packed", "brisk_hip_correct_reads",
    "brisk_hip_merge", "brisk_hip_intersect", "brisk_hip_subtract", "brisk_hip_compare", "brisk_hip_joint_spectrum", "brisk_hip_filter_joint", "brisk_hip_snapshot_info_read", "brisk_hip_save", "brisk_hip_load",
    "brisk_hip_adjacency", "brisk_hip_degree_spectrum", "brisk_hip_prune_degrees", "brisk_hip_graph_phase_ms",
    "brisk_hip_profile_enable",
    "brisk_hip_profile_read", "brisk_hip_profile_reset",
]

_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise BriskHipError(6, f"{path} is missing: run __graft_entry__.build() (no CPU fallback exists)")
    L = C.CDLL(path)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    L.brisk_hip_abi_version.restype = u32
    L.brisk_hip_create.argtypes = [C.POINTER(vp), C.c_uint8, C.c_uint8, C.c_uint8, u32, C.POINTER(C.c_double), C.POINTER(_Options)]
    L.brisk_hip_destroy.argtypes = [vp]
    L.brisk_hip_clear.argtypes = [vp]
    L.brisk_hip_last_error.argtypes = [vp]
    L.brisk_hip_last_error.restype = C.c_char_p
    L.brisk_hip_sync.argtypes = [vp]
    L.brisk_hip_get_layout.argtypes = [vp, C.POINTER(_Layout)]
    L.brisk_hip_get_minimizer_mode.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.brisk_hip_insert_reads.argtypes = [vp, _u8p, _u64p, u64]
    L.brisk_hip_insert_packed.argtypes = [vp, vp, vp, u64]
    L.brisk_hip_get_packed.argtypes = [vp, vp, vp, u64, vp]
    L.brisk_hip_get_reads.argtypes = [vp, _u8p, _u64p, u64, _u64p]
    L.brisk_hip_lookup.argtypes = [vp, _u64p, _u64p, _u8p, u64, _u8p, _u8p]
    _u16p = np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS")
    L.brisk_hip_get_kmers.argtypes = [vp, _u8p, _u64p, u64, _u16p, u64]
    L.brisk_hip_get_kmers_packed.argtypes = [vp, vp, vp, u64, vp]
    _profp = np.ctypeslib.ndpointer(dtype=READ_PROFILE_DTYPE, flags="C_CONTIGUOUS")
    L.brisk_hip_read_profile_reads.argtypes = [vp, _u8p, _u64p, u64, u32, _profp]
    L.brisk_hip_read_profile_packed.argtypes = [vp, vp, vp, u64, u32, vp]
    _ivp = np.ctypeslib.ndpointer(dtype=READ_INTERVAL_DTYPE, flags="C_CONTIGUOUS")
    L.brisk_hip_select_intervals.argtypes = [vp, vp, u64, C.POINTER(_SelectRule), vp]
    L.brisk_hip_extract_packed.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp, C.POINTER(u64), C.POINTER(u64)]
    L.brisk_hip_trim_packed.argtypes = [vp, vp, vp, u64, u32, C.POINTER(_SelectRule), vp, u64, vp, vp, C.POINTER(u64), C.POINTER(u64)]
    L.brisk_hip_trim_reads.argtypes = [vp, _u8p, _u64p, u64, u32, C.POINTER(_SelectRule), _ivp]
    L.brisk_hip_unpack_ascii.argtypes = [vp, vp, u64, u64, vp]
    _fragp = np.ctypeslib.ndpointer(dtype=FRAGMENT_DTYPE, flags="C_CONTIGUOUS")
    L.brisk_hip_intake_ascii.argtypes = [vp, vp, vp, vp, u64, C.POINTER(_IntakeRule), vp, u64, vp, vp, u64, C.POINTER(_IntakeStats)]
    L.brisk_hip_intake_reads.argtypes = [vp, vp, vp, _u64p, u64, C.POINTER(_IntakeRule), _fragp, u64, C.POINTER(_IntakeStats)]
    L.brisk_hip_insert_raw_reads.argtypes = [vp, vp, vp, _u64p, u64, C.POINTER(_IntakeRule), C.POINTER(_IntakeStats)]
    _pair_out4 = [vp, u64, vp, vp]  # one output stream: packed, cap_words, starts, index
    L.brisk_hip_fragment_intervals.argtypes = [vp, vp, u64, u64, vp]
    L.brisk_hip_pair_intervals.argtypes = [vp, vp, vp, u64, u32, vp]
    L.brisk_hip_compose_intervals.argtypes = [vp, vp, u64, vp, vp, u64, vp]
    L.brisk_hip_extract_pairs_packed.argtypes = [vp, vp, vp, u64, vp] + _pair_out4 * 2 + [C.POINTER(_PairCounts)]
    L.brisk_hip_trim_pairs_packed.argtypes = [vp, vp, vp, u64, u32, C.POINTER(_SelectRule), u32] + _pair_out4 * 2 + [C.POINTER(_PairCounts)]
    L.brisk_hip_trim_pairs_reads.argtypes = [vp, _u8p, _u64p, u64, u32, C.POINTER(_SelectRule), u32, _ivp, C.POINTER(_PairCounts)]
    L.brisk_hip_clean_pairs_ascii.argtypes = [vp, vp, vp, vp, u64, C.POINTER(_IntakeRule), C.POINTER(_SelectRule), u32, u32] + _pair_out4 * 2 + \
                                             [vp, C.POINTER(_PairCounts), C.POINTER(_IntakeStats)]
    L.brisk_hip_clean_pairs_reads.argtypes = [vp, vp, vp, _u64p, u64, C.POINTER(_IntakeRule), C.POINTER(_SelectRule), u32, u32, _ivp, C.POINTER(_PairCounts),
                                              C.POINTER(_IntakeStats)]
    L.brisk_hip_solid_runs.argtypes = [vp, vp, vp, u64, u32, u32, vp, u64, C.POINTER(_SplitStats)]
    L.brisk_hip_extract_fragments_packed.argtypes = [vp, vp, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64)]
    L.brisk_hip_split_packed.argtypes = [vp, vp, vp, u64, u32, u32, vp, u64, vp, vp, u64, C.POINTER(_SplitStats)]
    L.brisk_hip_split_reads.argtypes = [vp, _u8p, _u64p, u64, u32, u32, _fragp, u64, C.POINTER(_SplitStats)]
    _corrp = np.ctypeslib.ndpointer(dtype=CORRECTION_DTYPE, flags="C_CONTIGUOUS")
    L.brisk_hip_weak_sites.argtypes = [vp, vp, vp, u64, u32, u32, vp, u64, C.POINTER(_CorrectStats)]
    L.brisk_hip_candidate_windows.argtypes = [vp, vp, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64)]
    L.brisk_hip_decide_sites.argtypes = [vp, vp, vp, u64, vp, vp, u64, u32, vp, u64, C.POINTER(_CorrectStats)]
    L.brisk_hip_apply_corrections.argtypes = [vp, vp, vp, u64, vp, u64, vp, u64]
    L.brisk_hip_correct_packed.argtypes = [vp, vp, vp, u64, u32, u32, vp, u64, vp, u64, C.POINTER(_CorrectStats)]
    L.brisk_hip_correct_reads.argtypes = [vp, _u8p, _u64p, u64, u32, u32, _corrp, u64, C.POINTER(_CorrectStats)]
    L.brisk_hip_enumerate.argtypes = [vp, C.POINTER(u64), _u64p, _u64p, _u8p, _u8p, u64, C.POINTER(u64)]
    L.brisk_hip_stats.argtypes = [vp] + [C.POINTER(u64)] * 5
    L.brisk_hip_checksum.argtypes = [vp, _u64p]
    L.brisk_hip_memory_info.argtypes = [vp, _u64p]
    L.brisk_hip_insert_slack.argtypes = [vp, C.POINTER(u64)]
    L.brisk_hip_reallocate.argtypes = [vp, vp]
    L.brisk_hip_scan_packed.argtypes = [vp, vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.brisk_hip_scan_bound.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.brisk_hip_route_records.argtypes = [vp, vp, u64, vp, _u64p]
    L.brisk_hip_insert_records.argtypes = [vp, vp, u64]
    L.brisk_hip_set_owner_cuts.argtypes = [vp, _u64p]
    L.brisk_hip_export_hist.argtypes = [vp, vp, _u64p]
    L.brisk_hip_export_hist_add.argtypes = [vp, vp, _u64p]
    L.brisk_hip_insert_records_hist.argtypes = [vp, vp, u64, vp, u32]
    L.brisk_hip_scan_query.argtypes = [vp, vp, vp, u64, vp, vp, u64, C.POINTER(u64)]
    L.brisk_hip_route_tagged.argtypes = [vp, vp, vp, u64, vp, vp, _u64p]
    L.brisk_hip_query_records.argtypes = [vp, vp, u64, vp]
    L.brisk_hip_scan_kmers.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.brisk_hip_record_kmers.argtypes = [vp, vp, u64, vp]
    L.brisk_hip_answer_records.argtypes = [vp, vp, u64, vp, vp]
    L.brisk_hip_place_answers.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64]
    L.brisk_hip_profile_slots.argtypes = [vp, vp, vp, u64, u32, vp]
    L.brisk_hip_pack_ascii.argtypes = [vp, vp, u64, vp]
    L.brisk_hip_synth_reads.argtypes = [vp, u64, u64, u64, u32, u64, u64, vp, vp]
    _u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
    L.brisk_hip_scan_sequence.argtypes = [vp, C.c_char_p, u64, u64, _u64p, _u32p, _u64p, _u64p, _u8p, C.POINTER(u64)]
    L.brisk_hip_upsert_kmers.argtypes = [vp, _u64p, _u64p, _u8p, u64, _u32p, _u8p]
    L.brisk_hip_find_kmers.argtypes = [vp, _u64p, _u64p, _u8p, u64, _u32p]
    L.brisk_hip_enumerate_ids.argtypes = [vp, C.POINTER(u64), _u64p, _u64p, _u8p, _u32p, u64, C.POINTER(u64)]
    L.brisk_hip_count_spectrum.argtypes = [vp, _u64p]
    L.brisk_hip_enumerate_range.argtypes = [vp, C.POINTER(u64), _u64p, _u64p, _u8p, _u8p, u64, C.POINTER(u64), u32, u32]
    L.brisk_hip_prune.argtypes = [vp, u32, u32, C.POINTER(u64)]
    L.brisk_hip_adjacency.argtypes = [vp, u32, vp, u64, C.POINTER(u64)]
    L.brisk_hip_degree_spectrum.argtypes = [vp, u32, _u64p]
    L.brisk_hip_prune_degrees.argtypes = [vp, u32, u32, u32, C.POINTER(u64)]
    L.brisk_hip_graph_phase_ms.argtypes = [vp, np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")]
    L.brisk_hip_merge.argtypes = [vp, vp, C.POINTER(u64)]
    L.brisk_hip_intersect.argtypes = [vp, vp, u32, C.POINTER(u64)]
    L.brisk_hip_subtract.argtypes = [vp, vp, C.POINTER(u64)]
    L.brisk_hip_compare.argtypes = [vp, vp, _u64p]
    L.brisk_hip_joint_spectrum.argtypes = [vp, vp, vp]
    L.brisk_hip_filter_joint.argtypes = [vp, vp, C.POINTER(_JointWindow), C.POINTER(u64)]
    L.brisk_hip_snapshot_info_read.argtypes = [C.c_char_p, C.POINTER(_SnapshotInfo)]
    L.brisk_hip_save.argtypes = [vp, C.c_char_p, C.POINTER(u64)]
    L.brisk_hip_load.argtypes = [vp, C.c_char_p, u32, C.POINTER(u64)]
    L.brisk_hip_debug_order_keys.argtypes = [vp, _u64p, u64, i32, _u64p]
    L.brisk_hip_profile_enable.argtypes = [vp, i32]
    L.brisk_hip_profile_read.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_char_p), C.POINTER(u64), C.POINTER(C.c_double)]
    L.brisk_hip_profile_reset.argtypes = [vp]
    for s in SYMBOLS:
        if getattr(L, s).restype is C.c_int:
            pass
    _lib = L
    return L


def _pack_reads(seqs) -> Tuple[np.ndarray, np.ndarray]:
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    offs = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    flat = np.frombuffer(b"".join(bs), dtype=np.uint8).copy() if bs else np.zeros(0, np.uint8)
    return np.ascontiguousarray(flat), offs


def kmer_slots(offsets, k: int) -> np.ndarray:
    """Slot bases of brisk_hip_get_kmers: read r of the read table `offsets` (n_reads + 1 ascending nucleotide offsets) owns
    max(0, len_r - k + 1) slots from base[r]; base[n_reads] is the total, what `out` must hold."""
    offs = np.asarray(offsets, dtype=np.uint64)
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    base = np.zeros(len(offs), dtype=np.uint64)
    if len(lens):
        base[1:] = np.cumsum(np.maximum(lens - (k - 1), 0), dtype=np.uint64)
    return base


# brisk_hip_read_profile (include/brisk_hip.h): 32 bytes, little-endian, no padding
READ_PROFILE_DTYPE = np.dtype([("n_kmers", "<u4"), ("n_present", "<u4"), ("n_solid", "<u4"), ("run_start", "<u4"), ("run_len", "<u4"),
                               ("min_present", "u1"), ("max_present", "u1"), ("median", "u1"), ("median_present", "u1"), ("sum", "<u8")])
assert READ_PROFILE_DTYPE.itemsize == 32


def profile_from_slots(counts, found, base, solid_min: int) -> np.ndarray:
    """The record of brisk_hip_read_profile_reads computed on the host from the three outputs of BriskHip.get_kmers (counts
    uint8[n_slots], found bool[n_slots], base uint64[n_reads + 1]): the definition of every field, written out.  No device needed.
    A slot is solid when it is found and its count is >= solid_min (so none is when solid_min > 255); medians are lower medians,
    sorted[(n - 1) // 2]; `median` counts an absent slot as 0; the run is the first of the longest runs of consecutive solid slots."""
    counts = np.asarray(counts, np.uint8)
    found = np.asarray(found, bool)
    base = np.asarray(base, np.uint64).astype(np.int64)
    out = np.zeros(len(base) - 1, READ_PROFILE_DTYPE)
    for r in range(len(base) - 1):
        c, f = counts[base[r]:base[r + 1]].astype(np.int64), found[base[r]:base[r + 1]]
        n = len(c)
        if n > 0xffffffff:
            raise ValueError("a read of more than 2^32 - 1 slots does not fit the record")
        rec = out[r]
        rec["n_kmers"] = n
        if n == 0:
            continue
        present = c[f]
        solid = f & (c >= solid_min)
        rec["n_present"] = len(present)
        rec["n_solid"] = int(solid.sum())
        rec["median"] = np.sort(np.where(f, c, 0))[(n - 1) // 2]
        if len(present):
            rec["min_present"], rec["max_present"] = present.min(), present.max()
            rec["median_present"] = np.sort(present)[(len(present) - 1) // 2]
            rec["sum"] = int(present.sum())
        if solid.any():  # runs: where the padded mask rises and falls
            edge = np.diff(np.concatenate(([0], solid.astype(np.int8), [0])))
            starts, ends = np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]
            best = int(np.argmax(ends - starts))  # argmax returns the first of equal maxima
            rec["run_start"], rec["run_len"] = starts[best], ends[best] - starts[best]
    return out


# brisk_hip_read_interval (include/brisk_hip.h): nucleotides [start, start + len) of a read; len == 0: the read is dropped
READ_INTERVAL_DTYPE = np.dtype([("start", "<u4"), ("len", "<u4")])
assert READ_INTERVAL_DTYPE.itemsize == 8

# brisk_hip_select_rule.kind: BRISK_HIP_SELECT_SOLID_RUN / _MEDIAN / _PRESENT ("trim" is the command line's name for the first)
SELECT_KINDS = {"solid_run": 0, "trim": 0, "median": 1, "present": 2}


class _SelectRule(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "kind", "min_len", "lo", "hi")]


def select_rule(kind, min_len: int = 0, lo: int = 0, hi: int = 0xffffffff) -> _SelectRule:
    """A brisk_hip_select_rule: kind "solid_run" (the nucleotides the first longest run of solid k-mers covers), "median" (the whole
    read when lo <= median <= hi) or "present" (the whole read when lo <= 1000 * n_present / n_kmers <= hi, in permille), or the
    number of one; min_len: a kept interval has at least max(min_len, k) nucleotides.  Nothing is checked here: the library (EINVAL)
    and intervals_from_profile (ValueError) refuse an unknown kind and lo > hi."""
    return _SelectRule(C.sizeof(_SelectRule), SELECT_KINDS[kind] if isinstance(kind, str) else int(kind), min_len, lo, hi)


def intervals_from_profile(profile, k: int, rule) -> np.ndarray:
    """The rule of brisk_hip_select_intervals on the host: READ_INTERVAL_DTYPE[n] from READ_PROFILE_DTYPE[n] records, the handle's k
    and a select_rule(...).  The definition, written out; no device needed.  A read without k-mers is dropped (len 0), and so is an
    interval shorter than max(min_len, k) nucleotides or longer than 2^32 - 1."""
    if rule.struct_size < C.sizeof(_SelectRule) or rule.kind > 2 or rule.lo > rule.hi:
        raise ValueError("not a rule: struct_size %d kind %d lo %d hi %d" % (rule.struct_size, rule.kind, rule.lo, rule.hi))
    p = np.asarray(profile)
    assert p.dtype == READ_PROFILE_DTYPE
    n_kmers, lo, hi = p["n_kmers"].astype(np.int64), int(rule.lo), int(rule.hi)
    start = np.zeros(len(p), np.int64)
    if rule.kind == 0:
        keep = p["run_len"] >= 1
        start = np.where(keep, p["run_start"].astype(np.int64), 0)
        length = np.where(keep, p["run_len"].astype(np.int64) + k - 1, 0)
    else:
        if rule.kind == 1:
            keep = (p["median"] >= lo) & (p["median"] <= hi)
        else:  # (Python integers where a product can pass 2^63)
            n_present = p["n_present"].astype(np.int64)
            keep = np.array([lo * int(n) <= 1000 * int(q) <= hi * int(n) for n, q in zip(n_kmers, n_present)], bool)
        length = np.where(keep, n_kmers + k - 1, 0)
    keep = (n_kmers > 0) & (length >= max(int(rule.min_len), k)) & (length <= 0xffffffff)
    out = np.zeros(len(p), READ_INTERVAL_DTYPE)
    out["start"] = np.where(keep, start, 0)
    out["len"] = np.where(keep, length, 0)
    return out


# brisk_hip_fragment (include/brisk_hip.h): bytes [start, start + len) of read `read`; 16 bytes, little-endian, no padding
FRAGMENT_DTYPE = np.dtype([("read", "<u8"), ("start", "<u4"), ("len", "<u4")])
assert FRAGMENT_DTYPE.itemsize == 16
INTAKE_STATS_FIELDS = ("n_reads", "n_reads_kept", "n_fragments", "n_bases_in", "n_nts", "n_cut_base", "n_cut_qual", "n_short")
INTAKE_BLOCK = 4096  # BRISK_HIP_INTAKE_BLOCK: input bytes per thread block of the intake kernels


class _IntakeRule(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "min_len", "min_qual", "qual_base")]


class _IntakeStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in INTAKE_STATS_FIELDS]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n in INTAKE_STATS_FIELDS}


class _Fragment(C.Structure):
    _fields_ = [("read", C.c_uint64), ("start", C.c_uint32), ("len", C.c_uint32)]


def intake_rule(min_len: int = 0, min_qual: int = 0, qual_base: int = 33) -> _IntakeRule:
    """A brisk_hip_intake_rule: a fragment has at least max(min_len, k) nucleotides; a base whose quality byte is below qual_base +
    min_qual is cut like an N (min_qual 0: no quality cut); qual_base 33 or 64.  Nothing is checked here: the library (EINVAL) and
    fragments_from_reads (ValueError) refuse min_qual > 93 and any other qual_base."""
    return _IntakeRule(C.sizeof(_IntakeRule), min_len, min_qual, qual_base)


_IS_BASE = np.zeros(256, bool)
_IS_BASE[list(b"ACGTacgt")] = True


def _as_bytes_list(seqs) -> list:
    return [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]


def fragments_from_reads(seqs, quals, k: int, rule=None):
    """The rule of brisk_hip_intake_* on the host: (FRAGMENT_DTYPE[n_fragments], stats dict).  The definition, written out; no device
    needed.  A byte is valid when it is one of ACGTacgt and either min_qual == 0 or its quality byte >= qual_base + min_qual; a
    fragment is a maximal run of valid bytes inside one read, of at least max(min_len, k) bytes; fragments are ordered by read, then
    by position.  seqs[f.read][f.start:f.start + f.len] is fragment f's string."""
    rule = intake_rule() if rule is None else rule
    qual_base = rule.qual_base or 33
    if rule.struct_size < C.sizeof(_IntakeRule) or rule.min_qual > 93 or qual_base not in (33, 64):
        raise ValueError("not a rule: struct_size %d min_qual %d qual_base %d" % (rule.struct_size, rule.min_qual, rule.qual_base))
    bs = _as_bytes_list(seqs)
    qs = None if quals is None else _as_bytes_list(quals)
    if rule.min_qual and qs is None:
        raise ValueError("min_qual > 0 needs the qualities")
    if qs is not None and [len(q) for q in qs] != [len(b) for b in bs]:
        raise ValueError("a quality string differs in length from its read")
    min_len = max(int(rule.min_len), k)
    st = dict.fromkeys(INTAKE_STATS_FIELDS, 0)
    st["n_reads"] = len(bs)
    rows = []
    for r, b in enumerate(bs):
        a = np.frombuffer(b, np.uint8)
        base = _IS_BASE[a]
        valid = base
        if rule.min_qual:
            valid = base & (np.frombuffer(qs[r], np.uint8) >= qual_base + rule.min_qual)
        st["n_bases_in"] += len(a)
        st["n_cut_base"] += int((~base).sum())
        st["n_cut_qual"] += int((base & ~valid).sum())
        edge = np.diff(np.concatenate(([0], valid.astype(np.int8), [0])))
        starts, ends = np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]
        lens = ends - starts
        keep = lens >= min_len
        st["n_short"] += int(lens[~keep].sum())
        st["n_nts"] += int(lens[keep].sum())
        st["n_fragments"] += int(keep.sum())
        st["n_reads_kept"] += bool(keep.any())
        rows.extend((r, int(s), int(n)) for s, n in zip(starts[keep], lens[keep]))
    return np.array(rows, FRAGMENT_DTYPE) if rows else np.zeros(0, FRAGMENT_DTYPE), st


def _pack_raw(seqs, quals):
    """(flat bases, flat qualities or None, offsets) of str / bytes reads; ValueError where a quality string's length is not its read's"""
    bs = _as_bytes_list(seqs)
    flat, offs = _pack_reads(bs)
    qflat = None
    if quals is not None:
        qs = _as_bytes_list(quals)
        if len(qs) != len(bs) or any(len(q) != len(b) for q, b in zip(qs, bs)):
            raise ValueError("a quality string differs in length from its read")
        qflat, _ = _pack_reads(qs)
    return flat, qflat, offs


# ---- read splitting (include/brisk_hip.h, "read splitting"): every solid run of a read as a fragment of its own ----
SPLIT_STATS_FIELDS = ("n_reads", "n_reads_kept", "n_fragments", "n_slots", "n_solid", "n_short", "n_nts_in", "n_nts_out")


class _SplitStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in SPLIT_STATS_FIELDS]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n in SPLIT_STATS_FIELDS}


def fragments_from_slots(counts, found, base, k: int, solid_min: int = 2, min_len: int = 0, n_nts_in: Optional[int] = None):
    """The rule of brisk_hip_solid_runs / _split_* on the host: (FRAGMENT_DTYPE[n_fragments], stats dict) from the three outputs of
    BriskHip.get_kmers.  The definition, written out; no device needed.  A slot is solid when it is found and its count is >=
    solid_min (none is when solid_min > 255; every found one when it is 0); a run is a maximal stretch of consecutive solid slots of
    one read; a run of s slots from slot i on is the fragment {read, start = i, len = s + k - 1} when that length is at least
    max(min_len, k); fragments are ordered by read, then by start.  seqs[f.read][f.start:f.start + f.len] is fragment f's string.
    n_nts_in: the reads' nucleotides, which the slots do not tell for a read shorter than k (None: such a read counts as empty)."""
    counts = np.asarray(counts, np.uint8)
    solid = np.asarray(found, bool) & (counts.astype(np.int64) >= int(solid_min))
    base = np.asarray(base, np.uint64).astype(np.int64)
    n_reads = len(base) - 1
    min_nts = max(int(min_len), k)
    slots = base[1:] - base[:-1]
    st = dict.fromkeys(SPLIT_STATS_FIELDS, 0)
    st["n_reads"] = n_reads
    st["n_slots"] = int(base[-1]) if n_reads > 0 else 0
    st["n_nts_in"] = int((slots[slots > 0] + k - 1).sum()) if n_nts_in is None else int(n_nts_in)
    rows = []
    for r in range(n_reads):
        s = solid[base[r]:base[r + 1]]
        if not s.any():
            continue
        edge = np.diff(np.concatenate(([0], s.astype(np.int8), [0])))  # runs: where the padded mask rises and falls
        starts, ends = np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]
        lens = ends - starts
        keep = lens + k - 1 >= min_nts
        st["n_solid"] += int(lens.sum())
        st["n_short"] += int(lens[~keep].sum())
        st["n_nts_out"] += int((lens[keep] + k - 1).sum())
        st["n_fragments"] += int(keep.sum())
        st["n_reads_kept"] += bool(keep.any())
        rows.extend((r, int(a), int(n) + k - 1) for a, n in zip(starts[keep], lens[keep]))
    return np.array(rows, FRAGMENT_DTYPE) if rows else np.zeros(0, FRAGMENT_DTYPE), st


# ---- spectral read correction (include/brisk_hip.h, "spectral read correction"): isolated substitutions repaired ----
SITE_DTYPE = np.dtype([("read", "<u8"), ("pos", "<u4"), ("cover", "<u4")])
CORRECTION_DTYPE = np.dtype([("read", "<u8"), ("pos", "<u4"), ("from", "u1"), ("to", "u1"), ("cover", "<u2")])
assert SITE_DTYPE.itemsize == 16 and CORRECTION_DTYPE.itemsize == 16
CORRECT_STATS_FIELDS = ("n_reads", "n_slots", "n_weak", "n_runs", "n_sites", "n_skip_whole", "n_skip_long", "n_skip_short", "n_corrected", "n_ambiguous", "n_unresolved")


class _CorrectStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in CORRECT_STATS_FIELDS]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n in CORRECT_STATS_FIELDS}


def sites_from_slots(counts, found, base, k: int, solid_min: int = 2, min_cover: Optional[int] = None):
    """The rule of brisk_hip_weak_sites on the host: (SITE_DTYPE[n_sites], stats dict) from the three outputs of BriskHip.get_kmers.
    The definition, written out; no device needed.  A weak run is a maximal stretch [i, i + w) of slots of one read (n slots) that
    are not solid.  In this order: whole when i == 0 and i + w == n; long when w > k; short when it is interior (i > 0, i + w < n)
    with w < k, or when w < C (C = min_cover; None or 0: k); else the site {read, pos, cover = w}, pos = i + w - 1 when a solid slot
    follows the run and i + k - 1 when the run ends the read.  Sites are ordered by read, then by pos.  stats: CORRECT_STATS_FIELDS,
    the three decision counters zero.  ValueError when min_cover is above k."""
    counts = np.asarray(counts, np.uint8)
    weak = ~(np.asarray(found, bool) & (counts.astype(np.int64) >= int(solid_min)))
    base = np.asarray(base, np.uint64).astype(np.int64)
    c = int(min_cover) if min_cover else k
    if not 1 <= c <= k:
        raise ValueError("min_cover must be in 1..k (0 or None: k)")
    n_reads = len(base) - 1
    st = dict.fromkeys(CORRECT_STATS_FIELDS, 0)
    st["n_reads"] = n_reads
    st["n_slots"] = int(base[-1]) if n_reads > 0 else 0
    rows = []
    for r in range(n_reads):
        wk = weak[base[r]:base[r + 1]]
        n = len(wk)
        if not wk.any():
            continue
        edge = np.diff(np.concatenate(([0], wk.astype(np.int8), [0])))  # runs: where the padded mask rises and falls
        begins, ends = np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]
        st["n_weak"] += int((ends - begins).sum())
        st["n_runs"] += len(begins)
        for i, e in zip(begins.tolist(), ends.tolist()):
            w = e - i
            if i == 0 and e == n:
                st["n_skip_whole"] += 1
            elif w > k:
                st["n_skip_long"] += 1
            elif (i > 0 and e < n and w < k) or w < c:
                st["n_skip_short"] += 1
            else:
                st["n_sites"] += 1
                rows.append((r, e - 1 if e < n else i + k - 1, w))
    return np.array(rows, SITE_DTYPE) if rows else np.zeros(0, SITE_DTYPE), st


def site_windows(sites, k: int) -> np.ndarray:
    """The windows of a site table: FRAGMENT_DTYPE[n_sites] -- nucleotides [a, a + cover + k - 1) of the site's read, a = max(0, pos -
    k + 1).  The slots of a window are the slots of the site's weak run; candidate c of the site is the window with the base at
    pos - a replaced by the c-th of the three other codes of "ACTG" (codes 0..3), ascending."""
    t = np.asarray(sites)
    out = np.zeros(len(t), FRAGMENT_DTYPE)
    out["read"] = t["read"]
    out["start"] = np.maximum(t["pos"].astype(np.int64) - (k - 1), 0)
    out["len"] = t["cover"] + (k - 1)
    return out


def corrections_from_candidates(cand_counts, cand_found, sites, solid_min: int = 2, from_codes=None):
    """The rule of brisk_hip_decide_sites on the host: (CORRECTION_DTYPE[n_corrected], counts dict) from the slots of the candidate
    stream (BriskHip.get_kmers over the 3 * n_sites candidate strings: 3 * cover slots a site, in site order).  A candidate passes
    when all `cover` of its slots are solid; exactly one passes: a correction row; two or three: ambiguous; none: unresolved.
    from_codes[s]: the packed code (A0 C1 T2 G3) of the base at the site in the input; candidate c stands for the c-th of the three
    other codes, ascending, which becomes the row's `to` (None: from = 0 for every site).  counts: n_sites, n_corrected,
    n_ambiguous, n_unresolved."""
    t = np.asarray(sites)
    solid = np.asarray(cand_found, bool) & (np.asarray(cand_counts, np.uint8).astype(np.int64) >= int(solid_min))
    frm = np.zeros(len(t), np.int64) if from_codes is None else np.asarray(from_codes, np.int64)
    rows, at = [], 0
    cnt = {"n_sites": len(t), "n_corrected": 0, "n_ambiguous": 0, "n_unresolved": 0}
    for s in range(len(t)):
        cover = int(t["cover"][s])
        passing = [c for c in range(3) if solid[at + c * cover:at + (c + 1) * cover].all()]
        at += 3 * cover
        if len(passing) == 1:
            c, f = passing[0], int(frm[s])
            rows.append((int(t["read"][s]), int(t["pos"][s]), f, c + (c >= f), cover))
            cnt["n_corrected"] += 1
        elif passing:
            cnt["n_ambiguous"] += 1
        else:
            cnt["n_unresolved"] += 1
    if at != len(solid):
        raise ValueError("the candidate slots are not 3 * cover a site")
    return np.array(rows, CORRECTION_DTYPE) if rows else np.zeros(0, CORRECTION_DTYPE), cnt


# ---- paired-end reads (include/brisk_hip.h, "paired-end reads"): an interleaved stream, reads 2p and 2p + 1 the mates of pair p ----
# brisk_hip_pair_intervals' pair_mode: BRISK_HIP_PAIR_EACH / _ALL / _ANY
PAIR_MODES = {"each": 0, "all": 1, "any": 2}
PAIR_COUNTS_FIELDS = ("n_pairs_in", "n_pairs_kept", "n_single_first", "n_single_second", "n_pairs_dropped", "n_nts_pairs", "n_nts_singles", "reserved")


class _PairCounts(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in PAIR_COUNTS_FIELDS]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n in PAIR_COUNTS_FIELDS}


def _pair_mode(mode) -> int:
    m = PAIR_MODES.get(mode, -1) if isinstance(mode, str) else int(mode)
    if m not in (0, 1, 2):
        raise ValueError("unknown pair mode %r" % (mode,))
    return m


def intervals_from_fragments(frags, n_reads: int) -> np.ndarray:
    """brisk_hip_fragment_intervals on the host: READ_INTERVAL_DTYPE[n_reads] from an intake fragment table (FRAGMENT_DTYPE, ordered by
    read, then by position) -- {start, len} of the first longest fragment of every read, {0, 0} for a read without one.  The
    definition, written out; no device needed.  ValueError on a row with read >= n_reads and on a table that is not ordered."""
    f = np.asarray(frags)
    assert f.dtype == FRAGMENT_DTYPE
    read, start, length = f["read"].astype(np.int64), f["start"].astype(np.int64), f["len"].astype(np.int64)
    if len(f) and (f["read"] >= np.uint64(n_reads)).any():
        raise ValueError("row %d names a read >= n_reads" % int(np.nonzero(f["read"] >= np.uint64(n_reads))[0][0]))
    unordered = (read[1:] < read[:-1]) | ((read[1:] == read[:-1]) & (start[1:] <= start[:-1]))
    if unordered.any():
        raise ValueError("row %d stands before the row ahead of it" % (int(np.nonzero(unordered)[0][0]) + 1))
    out = np.zeros(n_reads, READ_INTERVAL_DTYPE)
    if len(f):
        order = np.lexsort((np.arange(len(f)), -length, read))  # by read; the longest first; of equal lengths the earliest row
        first = np.concatenate(([True], read[order][1:] != read[order][:-1]))
        best = order[first]
        out["start"][read[best]] = start[best]
        out["len"][read[best]] = length[best]
    return out


def pair_intervals(each, whole, mode) -> np.ndarray:
    """brisk_hip_pair_intervals on the host: the pair decision over interleaved READ_INTERVAL_DTYPE rows.  "each": the rows of `each`
    as they are; "all": a pair keeps both rows of `each` when both have len > 0, else both become {0, 0}; "any": when either mate's
    row of `each` has len > 0 both mates get their row of `whole` (one with len 0 stays {0, 0}), else both become {0, 0}.  `whole` is
    needed for "any" only.  ValueError on an odd number of rows, an unknown mode, "any" without `whole`."""
    m = _pair_mode(mode)
    e = np.asarray(each)
    assert e.dtype == READ_INTERVAL_DTYPE
    if len(e) % 2:
        raise ValueError("an interleaved stream holds whole pairs: %d rows" % len(e))
    out = e.copy()
    kept = (e["len"] > 0).reshape(-1, 2)
    if m == 1:
        out[np.repeat(~kept.all(axis=1), 2)] = (0, 0)
    elif m == 2:
        if whole is None:
            raise ValueError('"any" needs the whole-read intervals')
        w = np.asarray(whole)
        assert w.dtype == READ_INTERVAL_DTYPE and len(w) == len(e)
        out = w.copy()
        out[(w["len"] == 0) | np.repeat(~kept.any(axis=1), 2)] = (0, 0)
    return out


def compose_intervals(outer, inner, index) -> np.ndarray:
    """brisk_hip_compose_intervals on the host: two cuts chained.  outer[n_reads] is the first cut; inner[n_kept] a cut of the reads
    the first one kept; index[n_kept] (ascending) the input read behind each of those.  out[index[j]] = {outer.start + inner[j].start,
    inner[j].len} ({0, 0} when inner[j].len == 0), every other row {0, 0}.  ValueError where inner leaves outer (inner.start +
    inner.len > outer.len), where index[j] >= n_reads, and on an index that does not ascend."""
    o, i = np.asarray(outer), np.asarray(inner)
    idx = np.asarray(index, np.uint64)
    assert o.dtype == READ_INTERVAL_DTYPE and i.dtype == READ_INTERVAL_DTYPE and len(i) == len(idx)
    if len(idx) and (idx >= np.uint64(len(o))).any():
        raise ValueError("row %d: the index names a read >= n_reads" % int(np.nonzero(idx >= np.uint64(len(o)))[0][0]))
    idx = idx.astype(np.int64)
    if (idx[1:] <= idx[:-1]).any():
        raise ValueError("the index does not ascend at row %d" % (int(np.nonzero(idx[1:] <= idx[:-1])[0][0]) + 1))
    leaves = i["start"].astype(np.int64) + i["len"].astype(np.int64) > o["len"][idx].astype(np.int64)
    if leaves.any():
        raise ValueError("row %d: the inner interval leaves the outer one" % int(np.nonzero(leaves)[0][0]))
    out = np.zeros(len(o), READ_INTERVAL_DTYPE)
    keep = i["len"] > 0
    out["start"][idx[keep]] = o["start"][idx[keep]] + i["start"][keep]
    out["len"][idx[keep]] = i["len"][keep]
    return out


def split_pairs(intervals):
    """k_pair_split on the host: (iv_pairs, iv_singles, counts) of interleaved READ_INTERVAL_DTYPE rows -- the rows of intact pairs
    (both mates have len > 0) with every other row {0, 0}, the rows of singles (exactly one mate has) likewise, and the
    brisk_hip_pair_counts as a dict.  brisk_hip_extract_pairs_packed is, by definition, brisk_hip_extract_packed over each table."""
    v = np.asarray(intervals)
    assert v.dtype == READ_INTERVAL_DTYPE
    if len(v) % 2:
        raise ValueError("an interleaved stream holds whole pairs: %d rows" % len(v))
    kept = (v["len"] > 0).reshape(-1, 2)
    both, one = np.repeat(kept.all(axis=1), 2), np.repeat(kept.sum(axis=1) == 1, 2)
    iv_pairs, iv_singles = v.copy(), v.copy()
    iv_pairs[~both] = (0, 0)
    iv_singles[~(one & (v["len"] > 0))] = (0, 0)
    counts = dict.fromkeys(PAIR_COUNTS_FIELDS, 0)
    counts["n_pairs_in"] = len(kept)
    counts["n_pairs_kept"] = int(kept.all(axis=1).sum())
    counts["n_single_first"] = int((kept[:, 0] & ~kept[:, 1]).sum())
    counts["n_single_second"] = int((kept[:, 1] & ~kept[:, 0]).sum())
    counts["n_pairs_dropped"] = int((~kept.any(axis=1)).sum())
    counts["n_nts_pairs"] = int(iv_pairs["len"].astype(np.int64).sum())
    counts["n_nts_singles"] = int(iv_singles["len"].astype(np.int64).sum())
    return iv_pairs, iv_singles, counts


def _interleave(a, b, what="reads"):
    """mates as one interleaved list: `a` alone is interleaved already; with `b`, read i of `a` and read i of `b` are a pair"""
    if b is None:
        a = list(a)
        if len(a) % 2:
            raise ValueError("an interleaved list of %s holds whole pairs: %d" % (what, len(a)))
        return a
    a, b = list(a), list(b)
    if len(a) != len(b):
        raise ValueError("the two lists of %s differ in length: %d and %d" % (what, len(a), len(b)))
    return [x for pair in zip(a, b) for x in pair]


_ONE_BYTE = np.zeros(1, np.uint8)  # what an empty array's pointer stands on: it lives as long as the module


def _host_ptr(a):
    """the address of a numpy array's bytes (of _ONE_BYTE for an empty one: a non-null pointer of which nothing is read), or None"""
    return None if a is None else C.c_void_p(a.ctypes.data if len(a) else _ONE_BYTE.ctypes.data)


def _pair_out(out):
    """(d_out_packed, out_cap_words, d_out_starts, d_out_index) of one output stream of the pairs calls as ctypes arguments; None: all null"""
    if out is None:
        return None, 0, None, None
    d_packed, cap, d_starts, d_index = out
    return d_packed or None, cap, d_starts or None, d_index or None


def joint_spectrum_from_entries(dump_a, dump_b) -> np.ndarray:
    """BriskHip.joint_spectrum on the host, from two (lo, hi, minimizer_idx, count) tuples as BriskHip.enumerate returns them: the
    definition, written out; no device needed.  The identity of an entry is (hi, lo, minimizer_idx) -- the same k-mer under two
    minimizer positions is two identities -- and each dump holds an identity once."""
    def keyed(dump):
        lo, hi, idx, cnt = (np.asarray(x) for x in dump)
        key = np.zeros(len(lo), np.dtype([("hi", "<u8"), ("lo", "<u8"), ("idx", "u1")]))
        key["hi"], key["lo"], key["idx"] = hi, lo, idx
        return key, cnt.astype(np.int64)
    (ka, ca), (kb, cb) = keyed(dump_a), keyed(dump_b)
    out = np.zeros((JOINT_STATES, JOINT_STATES), np.uint64)
    _, ia, ib = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)
    in_b = np.full(len(ka), JOINT_ABSENT, np.int64)  # every entry of a: its state in b
    in_b[ia] = cb[ib]
    np.add.at(out, (ca, in_b), 1)
    only_b = np.ones(len(kb), bool)
    only_b[ib] = False
    np.add.at(out, (np.full(int(only_b.sum()), JOINT_ABSENT), cb[only_b]), 1)
    return out


def joint_figures(joint, k: int, solid_min: int = 2) -> dict:
    """The usual figures off a joint spectrum, `self` (rows) read as the assembly and `other` (columns) as the reads -- host
    arithmetic only.  shared / only_self / only_other: entries in both, only in self, only in other.  completeness: the entries
    of other with count >= solid_min that are present in self, over all entries of other with count >= solid_min (nan when there
    are none).  error_rate = 1 - (1 - only_self / entries_of_self) ** (1 / k): the per-base error that would leave that share of
    self's k-mers without support (nan for an empty self); qv = -10 log10(error_rate), inf at 0.  Everything counts DISTINCT
    entries, not multiplicities: an entry seen 40 times weighs what an entry seen once does."""
    J = np.asarray(joint)
    if J.shape != (JOINT_STATES, JOINT_STATES):
        raise ValueError(f"a joint spectrum is {JOINT_STATES} x {JOINT_STATES}, not {J.shape}")
    A = JOINT_ABSENT
    shared, only_self, only_other = int(J[:A, :A].sum()), int(J[:A, A].sum()), int(J[A, :A].sum())
    lo = min(max(int(solid_min), 0), A)
    solid, solid_in_self = int(J[:, lo:A].sum()), int(J[:A, lo:A].sum())
    entries_self = shared + only_self
    error_rate = 1.0 - (1.0 - only_self / entries_self) ** (1.0 / k) if entries_self else float("nan")
    qv = float("inf") if error_rate == 0 else -10.0 * math.log10(error_rate) if error_rate > 0 else float("nan")
    return dict(shared=shared, only_self=only_self, only_other=only_other, completeness=solid_in_self / solid if solid else float("nan"),
                error_rate=error_rate, qv=qv)


# ---- de Bruijn adjacency (brisk_hip_adjacency / _degree_spectrum / _prune_degrees): the definition on the host
DEGREE_CLASSES = 26  # 5 * left + right for left, right in 0..4, and 25: "below min_count, not a node"


def degree_class(left: int, right: int) -> int:
    """The class of a node with `left` neighbours on its left and `right` on its right (0..4 each): the index into
    BriskHip.degree_spectrum and the bit of a prune_degrees mask."""
    if not (0 <= left <= 4 and 0 <= right <= 4):
        raise ValueError(f"a side has 0..4 neighbours, not ({left}, {right})")
    return 5 * left + right


def neighbour_strings(lo, hi, k: int) -> list:
    """The 8 * n neighbour strings of n entries as BriskHip.enumerate returns them (lo, hi: kmer_s, leftmost nucleotide in the
    highest bits, codes of "ACTG"): for entry i with string x, rows 8 i .. 8 i + 3 are R_c = x[1:] + c and rows 8 i + 4 .. 8 i + 7 are
    L_c = c + x[:-1], c = "ACTG"[0..3].  A list of bytes objects, what get_kmers takes.  No device needed."""
    lo, hi = np.asarray(lo, np.uint64), np.asarray(hi, np.uint64)
    n = len(lo)
    codes = np.zeros((n, k), np.uint8)
    for j in range(k):  # nucleotide j from the left: bits [2 (k - 1 - j), 2 (k - j)) of hi:lo
        sh = 2 * (k - 1 - j)
        codes[:, j] = ((lo >> np.uint64(sh)) if sh < 64 else (hi >> np.uint64(sh - 64))) & np.uint64(3)
    out = np.zeros((n, 8, k), np.uint8)
    for c in range(4):
        out[:, c, : k - 1] = codes[:, 1:]
        out[:, c, k - 1] = c
        out[:, 4 + c, 1:] = codes[:, : k - 1]
        out[:, 4 + c, 0] = c
    flat = np.frombuffer(b"ACTG", np.uint8)[out].tobytes()
    return [flat[i * k:(i + 1) * k] for i in range(8 * n)]


def adjacency_from_slots(counts, found, min_count: int = 0) -> np.ndarray:
    """The adjacency bytes from the slots of the neighbour strings (counts uint8[8 n], found bool[8 n], as BriskHip.get_kmers
    returns them for neighbour_strings(...)): bit j of byte i is set when slot 8 i + j is found and its count is >= min_count.
    adjacency_from_slots(*h.get_kmers(neighbour_strings(lo, hi, k))[:2], min_count) is by definition h.adjacency(min_count)."""
    counts, found = np.asarray(counts, np.uint8), np.asarray(found, bool)
    if len(counts) != len(found) or len(counts) % 8:
        raise ValueError("eight slots an entry")
    ok = (found & (counts.astype(np.int64) >= int(min_count))).reshape(-1, 8).astype(np.uint8)
    return (ok << np.arange(8, dtype=np.uint8)).sum(axis=1).astype(np.uint8)


_POP4 = np.array([bin(i).count("1") for i in range(16)], np.int64)


def degree_spectrum_from_adjacency(adj, counts, min_count: int = 0) -> np.ndarray:
    """BriskHip.degree_spectrum on the host, from the adjacency bytes and the entries' own counts (row for row, as enumerate
    returns them): uint64[26].  A node is an entry whose count is >= min_count; out[5 * left + right] counts the nodes with `left`
    set bits among bits 4..7 and `right` among bits 0..3; out[25] the entries that are no nodes.  The values sum to len(adj)."""
    adj, counts = np.asarray(adj, np.uint8), np.asarray(counts, np.uint8)
    if len(adj) != len(counts):
        raise ValueError("one byte and one count an entry")
    node = counts.astype(np.int64) >= int(min_count)
    cls = np.where(node, 5 * _POP4[adj >> 4] + _POP4[adj & 15], DEGREE_CLASSES - 1)
    return np.bincount(cls, minlength=DEGREE_CLASSES).astype(np.uint64)


def graph_figures(spectrum) -> dict:
    """The usual figures off a degree spectrum -- host arithmetic only.  nodes; edge_ends (the sum of all degrees: every edge between
    two nodes is seen from both of its ends); isolated (0, 0); dead_ends (exactly one side empty); simple (1, 1); branching (a side
    above 1); below (entries under min_count, not nodes).  Symmetric in left and right."""
    s = np.asarray(spectrum)
    if s.shape != (DEGREE_CLASSES,):
        raise ValueError(f"a degree spectrum has {DEGREE_CLASSES} values, not {s.shape}")
    m = s[:25].astype(np.int64).reshape(5, 5)
    left, right = np.arange(5)[:, None], np.arange(5)[None, :]
    return dict(nodes=int(m.sum()), edge_ends=int((m * (left + right)).sum()), isolated=int(m[0, 0]),
                dead_ends=int(m[(left == 0) != (right == 0)].sum()), simple=int(m[1, 1]),
                branching=int(m[(left > 1) | (right > 1)].sum()), below=int(s[25]))


def degree_mask(classes) -> int:
    """a prune_degrees mask from a mask or an iterable of (left, right) pairs"""
    if isinstance(classes, (int, np.integer)):
        return int(classes)
    mask = 0
    for left, right in classes:
        mask |= 1 << degree_class(left, right)
    return mask


def snapshot_info(path) -> dict:
    """The header of a snapshot file (brisk_hip_snapshot_info_read; host only: no device, no handle): k, m, b, data_bytes, part_bits,
    ext_bits, cls_bits, cls_width, key_words, shift, n_entries, n_partitions (the non-empty ones), nb_skmers, checksum (the three
    words of BriskHip.checksum at save time), n_blocks, version, header_bytes, file_bytes, count_mode (0 wrap, 1 saturate: COUNT_MODES)
    and minimizer_mode (0 reference, 1 full: MINIMIZER_MODES; 0 in files from before the field existed)."""
    info = _SnapshotInfo(C.sizeof(_SnapshotInfo))
    rc = load().brisk_hip_snapshot_info_read(os.fsencode(path), C.byref(info))
    if rc:
        raise BriskHipError(rc, f"snapshot_info({os.fspath(path)!r})")
    out = {n: getattr(info, n) for n, _ in _SnapshotInfo._fields_ if n not in ("struct_size", "checksum")}
    out["checksum"] = tuple(int(x) for x in info.checksum)
    return out


_live = weakref.WeakSet()


@atexit.register
def _close_all_handles():
    # destroy device state while the HIP runtime is still up: finalisers that run during
    # interpreter teardown would call into a runtime that may already be gone
    for ix in list(_live):
        try:
            ix.close()
        except Exception:
            pass


class BriskHip:
    """One index handle.  Methods map one-to-one onto the C-ABI.

    count_mode: "wrap" (the default: the count byte wraps at 256, as the reference's) or "saturate": an entry's count is
    min(255, the times its identity was inserted) -- 255 means "255 or more" and no present entry has count 0.  The mode is fixed
    at create time (the attribute `count_mode`), travels with snapshots, and two indexes of a set operation must agree in it.

    minimizer_mode: "reference" (the default: the reference's get_minimizer as executed -- at k > 32 its re-scan reads the last 32
    nucleotides of the k-mer only, and one canonical k-mer enters the index under several identities, its count split among them)
    or "full": the re-scan sees the whole k-mer, everything else is the reference's algorithm.  For k <= 32 both build the same
    index bit for bit.  Fixed at create time (the attribute `minimizer_mode`), it travels with snapshots (`open` creates the handle
    in the file's mode, `load` refuses the other one), every scan of the handle follows it, and the two indexes of merge, intersect,
    subtract, compare, joint_spectrum, filter_joint and reallocate must agree in it (EINVAL, the message names minimizer_mode)."""

    def __init__(self, k: int, m: int, b: int, device: int = 0, stream: Optional[int] = None, part_bits: int = 0,
                 owner_rank: int = 0, n_owners: int = 1, arena_entries: int = 0, max_batch_reads: int = 0,
                 entry_ids: bool = False, immediate_inserts: bool = False, count_mode: str = "wrap",
                 minimizer_mode: str = "reference"):
        if count_mode not in COUNT_MODES:
            raise ValueError(f"count_mode must be one of {sorted(COUNT_MODES)}, not {count_mode!r}")
        if minimizer_mode not in MINIMIZER_MODES:
            raise ValueError(f"minimizer_mode must be one of {sorted(MINIMIZER_MODES)}, not {minimizer_mode!r}")
        self.L = load()
        self.h = C.c_void_p()
        self.k, self.m, self.b = k, m, b
        self.device = device
        opt = _Options(C.sizeof(_Options), device, stream, part_bits, owner_rank, n_owners, MINIMIZER_MODES[minimizer_mode], arena_entries,
                       max_batch_reads, 1 if entry_ids else 0, 1 if immediate_inserts else 0, COUNT_MODES[count_mode])
        coef = coef_table(m) if 1 <= m <= 31 else np.zeros(4, np.float64)
        rc = self.L.brisk_hip_create(C.byref(self.h), k, m, b, 1, coef.ctypes.data_as(C.POINTER(C.c_double)), C.byref(opt))
        if rc:
            self.h = C.c_void_p()
            raise BriskHipError(rc, f"create(k={k},m={m},b={b})")
        _live.add(self)
        lay = _Layout()
        self._chk(self.L.brisk_hip_get_layout(self.h, C.byref(lay)))
        self.layout = {n: getattr(lay, n) for n, _ in _Layout._fields_}
        self.record_words = lay.record_words
        self.count_mode = {v: n for n, v in COUNT_MODES.items()}[lay.count_mode]
        mode = C.c_uint32()
        self._chk(self.L.brisk_hip_get_minimizer_mode(self.h, C.byref(mode)))
        self.layout["minimizer_mode"] = mode.value  # (brisk_hip_get_minimizer_mode: brisk_hip_layout cannot grow)
        self.minimizer_mode = {v: n for n, v in MINIMIZER_MODES.items()}[mode.value]

    def _chk(self, rc: int):
        if rc:
            raise BriskHipError(rc, (self.L.brisk_hip_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.brisk_hip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        if sys is None or sys.is_finalizing():  # module globals are already gone late in interpreter shutdown
            return
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- bulk host paths
    def insert_reads(self, seqs: Sequence) -> None:
        flat, offs = _pack_reads(seqs)
        self.insert_flat(flat, offs)

    def insert_flat(self, flat: np.ndarray, offs: np.ndarray) -> None:
        if len(flat) == 0:
            flat = np.zeros(1, np.uint8)
        self._chk(self.L.brisk_hip_insert_reads(self.h, flat, offs, len(offs) - 1))

    def get_reads(self, seqs: Sequence) -> np.ndarray:
        flat, offs = _pack_reads(seqs)
        out = np.zeros(len(offs) - 1, np.uint64)
        if len(flat) == 0:
            flat = np.zeros(1, np.uint8)
        self._chk(self.L.brisk_hip_get_reads(self.h, flat, offs, len(offs) - 1, out))
        return out

    def get_kmers(self, seqs: Sequence) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The count at every k-mer position (brisk_hip_get_kmers): counts uint8[n_slots] (mod 256; in a saturating index 1..255 where
        found, 255 meaning "255 or more"), found bool[n_slots], base uint64[n_reads + 1] -- the k-mer at nucleotide i of read r is
        slot base[r] + i."""
        flat, offs = _pack_reads(seqs)
        base = kmer_slots(offs, self.k)
        total = int(base[-1])
        out = np.zeros(max(total, 1), np.uint16)
        if len(flat) == 0:
            flat = np.zeros(1, np.uint8)
        self._chk(self.L.brisk_hip_get_kmers(self.h, flat, offs, len(offs) - 1, out, total))
        out = out[:total]
        return (out & 0xff).astype(np.uint8), (out & 0x100) != 0, base

    def read_profile(self, seqs: Sequence, solid_min: int = 2) -> np.ndarray:
        """One abundance record per read (brisk_hip_read_profile_reads): READ_PROFILE_DTYPE[n_reads] -- n_kmers, n_present, n_solid
        (present and count >= solid_min), the first longest run of solid slots (run_start, run_len), min / max / lower median of
        the present counts, the lower median over all slots (absent = 0) and the sum.  What profile_from_slots(*get_kmers(seqs),
        solid_min) gives, reduced on the device: the slots never reach the host.  Counts are the stored bytes: in a wrapping index an
        entry seen 256 times is present with count 0 and pulls a median down; in a saturating index (count_mode="saturate") counts stop
        at 255, which stands for "255 or more" in min / max / medians and the sum."""
        flat, offs = _pack_reads(seqs)
        out = np.zeros(len(offs) - 1, READ_PROFILE_DTYPE)
        if len(flat) == 0:
            flat = np.zeros(1, np.uint8)
        self._chk(self.L.brisk_hip_read_profile_reads(self.h, flat, offs, len(offs) - 1, solid_min, out if len(out) else np.zeros(1, READ_PROFILE_DTYPE)))
        return out

    def trim_reads(self, seqs: Sequence, solid_min: int = 2, rule: Optional[_SelectRule] = None) -> np.ndarray:
        """One interval per read (brisk_hip_trim_reads): READ_INTERVAL_DTYPE[n_reads] -- what intervals_from_profile(read_profile(seqs,
        solid_min), k, rule) gives, computed on the device; seqs[i][start:start + len] is what the rule keeps of read i, and len == 0
        means that the read is dropped.  rule: a select_rule(...); the default is select_rule("solid_run")."""
        flat, offs = _pack_reads(seqs)
        out = np.zeros(max(len(offs) - 1, 1), READ_INTERVAL_DTYPE)
        if len(flat) == 0:
            flat = np.zeros(1, np.uint8)
        rule = select_rule("solid_run") if rule is None else rule
        self._chk(self.L.brisk_hip_trim_reads(self.h, flat, offs, len(offs) - 1, solid_min, C.byref(rule), out))
        return out[:len(offs) - 1]

    def split_reads(self, seqs: Sequence, solid_min: int = 2, min_len: int = 0):
        """Every read cut at its weak k-mers (brisk_hip_split_reads): (FRAGMENT_DTYPE[n_fragments], stats dict) -- what
        fragments_from_slots(*get_kmers(seqs), k, solid_min, min_len) gives, computed on the device: one fragment per run of solid
        k-mers that covers at least max(min_len, k) nucleotides.  seqs[f.read][f.start:f.start + f.len] is fragment f's string; two
        fragments of one read may overlap by up to k - 2 nucleotides.  stats: SPLIT_STATS_FIELDS."""
        flat, offs = _pack_reads(seqs)
        cap = max(1, (int(kmer_slots(offs, self.k)[-1]) + len(offs)) // 2)  # a read of n slots has at most (n + 1) / 2 runs
        out = np.zeros(cap, FRAGMENT_DTYPE)
        if len(flat) == 0:
            flat = np.zeros(1, np.uint8)
        st = _SplitStats()
        self._chk(self.L.brisk_hip_split_reads(self.h, flat, offs, len(offs) - 1, solid_min, min_len, out, cap, C.byref(st)))
        return out[:st.n_fragments].copy(), st.as_dict()

    def correct_reads(self, seqs: Sequence, solid_min: int = 2, min_cover: Optional[int] = None):
        """Isolated substitutions found and decided on the device (brisk_hip_correct_reads): (CORRECTION_DTYPE[n_corrected], stats
        dict) -- a row says that nucleotide pos of read `read` holds code `from` and should hold code `to` (codes of "ACTG"); the
        caller patches its own strings.  What sites_from_slots, the candidate strings, get_kmers over them and
        corrections_from_candidates give, computed on the device.  min_cover (None or 0: k): the fewest weak k-mers a run at a
        read's edge may have and still be attempted.  stats: CORRECT_STATS_FIELDS."""
        flat, offs = _pack_reads(seqs)
        cap = max(1, (int(kmer_slots(offs, self.k)[-1]) + len(offs)) // 2)  # a read of n slots has at most (n + 1) / 2 weak runs
        out = np.zeros(cap, CORRECTION_DTYPE)
        if len(flat) == 0:
            flat = np.zeros(1, np.uint8)
        st = _CorrectStats()
        self._chk(self.L.brisk_hip_correct_reads(self.h, flat, offs, len(offs) - 1, solid_min, int(min_cover or 0), out, cap, C.byref(st)))
        return out[:st.n_corrected].copy(), st.as_dict()

    def intake(self, seqs: Sequence, quals: Optional[Sequence] = None, rule: Optional[_IntakeRule] = None):
        """The fragments of raw reads (brisk_hip_intake_reads): (FRAGMENT_DTYPE[n_fragments], stats dict) -- what
        fragments_from_reads(seqs, quals, k, rule) gives, computed on the device: maximal runs of ACGTacgt (at or above the quality
        threshold) inside one read, at least max(rule.min_len, k) long.  seqs[f.read][f.start:f.start + f.len] is fragment f's string.
        seqs and quals are str or bytes; ValueError where a quality string's length is not its read's.  Needs no index state."""
        flat, qflat, offs = _pack_raw(seqs, quals)
        rule = intake_rule() if rule is None else rule
        st = _IntakeStats()
        cap = max(1, len(flat) // max(1, max(int(rule.min_len), self.k)))
        out = np.zeros(cap, FRAGMENT_DTYPE)
        self._chk(self.L.brisk_hip_intake_reads(self.h, _host_ptr(flat), _host_ptr(qflat), offs, len(offs) - 1, C.byref(rule), out, cap, C.byref(st)))
        return out[:st.n_fragments].copy(), st.as_dict()

    def insert_raw(self, seqs: Sequence, quals: Optional[Sequence] = None, rule: Optional[_IntakeRule] = None) -> dict:
        """Count raw reads (brisk_hip_insert_raw_reads): the bytes go to the device as they are, are cut there at every byte that is not
        a base (and, with rule.min_qual, at every base below the quality threshold), and the fragments are inserted.  The index is the
        one insert_reads builds from the fragments' strings.  Returns the intake's stats.  Clean input should stay on insert_reads,
        which sends 2 bits per nucleotide to the device where this sends 8, or 16 with qualities."""
        flat, qflat, offs = _pack_raw(seqs, quals)
        rule = intake_rule() if rule is None else rule
        st = _IntakeStats()
        self._chk(self.L.brisk_hip_insert_raw_reads(self.h, _host_ptr(flat), _host_ptr(qflat), offs, len(offs) - 1, C.byref(rule), C.byref(st)))
        return st.as_dict()

    def trim_pairs(self, seqs1: Sequence, seqs2: Optional[Sequence] = None, solid_min: int = 2, rule: Optional[_SelectRule] = None, pair_mode="each"):
        """trim_reads for paired reads (brisk_hip_trim_pairs_reads): (READ_INTERVAL_DTYPE[n_reads], counts dict).  seqs1 alone is an
        interleaved list (reads 2p and 2p + 1 are mates); with seqs2, read i of each list are mates and the result is interleaved.  The
        intervals are pair_intervals(each, whole, pair_mode) of what trim_reads gives for every read alone ("any": a pair of which
        either mate passes keeps both mates whole); counts is split_pairs' (PAIR_COUNTS_FIELDS).  The caller slices its own strings."""
        seqs = _interleave(seqs1, seqs2)
        flat, offs = _pack_reads(seqs)
        out = np.zeros(max(len(seqs), 1), READ_INTERVAL_DTYPE)
        if len(flat) == 0:
            flat = np.zeros(1, np.uint8)
        rule = select_rule("solid_run") if rule is None else rule
        pc = _PairCounts()
        self._chk(self.L.brisk_hip_trim_pairs_reads(self.h, flat, offs, len(seqs), solid_min, C.byref(rule), _pair_mode(pair_mode), out, C.byref(pc)))
        return out[:len(seqs)], pc.as_dict()

    def clean_pairs(self, seqs1: Sequence, seqs2: Optional[Sequence] = None, quals1: Optional[Sequence] = None, quals2: Optional[Sequence] = None,
                    intake: Optional[_IntakeRule] = None, rule: Optional[_SelectRule] = None, solid_min: int = 2, pair_mode="each"):
        """Raw paired reads to one clean interval per read (brisk_hip_clean_pairs_reads): (READ_INTERVAL_DTYPE[n_reads], counts dict,
        intake stats dict).  Mates are given as in trim_pairs; qualities likewise.  The first longest fragment of a read under the
        intake rule is the read's; with `rule` (a select_rule) it is cut again by abundance, and the cut is expressed in the raw read's
        frame; then the pair decision.  seqs[i][start:start + len] holds only ACGTacgt.  Without `rule` no index state is needed."""
        seqs = _interleave(seqs1, seqs2)
        quals = None if quals1 is None else _interleave(quals1, quals2, "qualities")
        flat, qflat, offs = _pack_raw(seqs, quals)
        intake = intake_rule() if intake is None else intake
        out = np.zeros(max(len(seqs), 1), READ_INTERVAL_DTYPE)
        pc, st = _PairCounts(), _IntakeStats()
        self._chk(self.L.brisk_hip_clean_pairs_reads(self.h, _host_ptr(flat), _host_ptr(qflat), offs, len(seqs), C.byref(intake), C.byref(rule) if rule is not None else None,
                                                     solid_min, _pair_mode(pair_mode), out, C.byref(pc), C.byref(st)))
        return out[:len(seqs)], pc.as_dict(), st.as_dict()

    def lookup(self, lo, hi, idx) -> Tuple[np.ndarray, np.ndarray]:
        lo = np.ascontiguousarray(lo, np.uint64)
        hi = np.ascontiguousarray(hi, np.uint64)
        idx = np.ascontiguousarray(idx, np.uint8)
        n = len(lo)
        data = np.zeros(max(n, 1), np.uint8)
        found = np.zeros(max(n, 1), np.uint8)
        self._chk(self.L.brisk_hip_lookup(self.h, lo, hi, idx, n, data, found))
        return data[:n], found[:n]

    def enumerate(self, chunk: int = 1 << 20, min_count: int = 0, max_count: int = 255):
        """All entries: (lo, hi, minimizer_idx, count) arrays, k-mers unhashed.  With bounds other than the defaults: the
        entries whose count is in [min_count, max_count] only (brisk_hip_enumerate_range), in the same order."""
        ranged = (min_count, max_count) != (0, 255)
        cur = C.c_uint64(0)
        n = C.c_uint64(0)
        los, his, idxs, cnts = [], [], [], []
        cap = chunk
        while True:
            lo = np.zeros(cap, np.uint64)
            hi = np.zeros(cap, np.uint64)
            idx = np.zeros(cap, np.uint8)
            cnt = np.zeros(cap, np.uint8)
            if ranged:
                rc = self.L.brisk_hip_enumerate_range(self.h, C.byref(cur), lo, hi, idx, cnt, cap, C.byref(n), min_count, max_count)
            else:
                rc = self.L.brisk_hip_enumerate(self.h, C.byref(cur), lo, hi, idx, cnt, cap, C.byref(n))
            if rc == ECAPACITY:
                cap *= 4
                continue
            self._chk(rc)
            if n.value == 0:
                break
            los.append(lo[: n.value]); his.append(hi[: n.value]); idxs.append(idx[: n.value]); cnts.append(cnt[: n.value])
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
        return cat(los, np.uint64), cat(his, np.uint64), cat(idxs, np.uint8), cat(cnts, np.uint8)

    def count_spectrum(self) -> np.ndarray:
        """uint64[256]: out[c] = entries whose stored count (mod 256) is c.  In a saturating index (count_mode="saturate") bin 0 is
        empty and bin 255 holds the entries seen 255 times or more."""
        out = np.zeros(256, np.uint64)
        self._chk(self.L.brisk_hip_count_spectrum(self.h, out))
        return out

    def prune(self, min_count: int, max_count: int = 255) -> int:
        """remove, in place, every entry whose count is outside [min_count, max_count]; returns how many were removed.  The stored
        byte is compared: a wrapping index loses an entry seen 256 or 257 times to prune(2, 255); a saturating one
        (count_mode="saturate") holds it at 255 = "255 or more" and keeps it."""
        v = C.c_uint64()
        self._chk(self.L.brisk_hip_prune(self.h, min_count, max_count, C.byref(v)))
        return v.value

    # ---- de Bruijn adjacency: at k > 32 the graph wants a minimizer_mode="full" index
    def adjacency_device(self, d_adj: int, cap: int, min_count: int = 0) -> int:
        """One adjacency byte per entry into the caller's device buffer of `cap` bytes (brisk_hip_adjacency), in enumerate()'s order;
        returns the number of entries.  Bit c: x[1:] + "ACTG"[c] is present with count >= min_count; bit 4 + c: "ACTG"[c] + x[:-1] is.
        BriskHipError(ECAPACITY), with nothing written, when cap is too small."""
        n = C.c_uint64()
        self._chk(self.L.brisk_hip_adjacency(self.h, min_count, d_adj or None, cap, C.byref(n)))
        return n.value

    def adjacency(self, min_count: int = 0) -> np.ndarray:
        """uint8[n_entries], aligned with enumerate(): row i's neighbours (adjacency_device through a device buffer of its own)."""
        import torch  # the device buffer only; the bytes are the library's

        n = self.stats()["nb_kmers"]
        buf = torch.zeros(max(n, 1), dtype=torch.uint8, device=f"cuda:{self.device}")
        torch.cuda.synchronize(self.device)
        got = self.adjacency_device(buf.data_ptr(), n, min_count)
        return buf[:got].cpu().numpy()

    def degree_spectrum(self, min_count: int = 0) -> np.ndarray:
        """uint64[26]: out[degree_class(left, right)] = the nodes (entries with count >= min_count) with that many neighbours on each
        side, out[25] = the entries below min_count.  Sums to nb_kmers.  graph_figures reads it."""
        out = np.zeros(DEGREE_CLASSES, np.uint64)
        self._chk(self.L.brisk_hip_degree_spectrum(self.h, min_count, out))
        return out

    def prune_degrees(self, classes, min_count: int = 0, max_count: int = 255) -> int:
        """remove, in place, every node (count >= min_count) of count <= max_count whose degree class is in `classes` -- a mask of
        1 << degree_class(left, right) bits or an iterable of (left, right) pairs; returns how many were removed.  The graph is taken
        once, before anything is removed.  Everything prune() promises holds afterwards."""
        v = C.c_uint64()
        self._chk(self.L.brisk_hip_prune_degrees(self.h, min_count, max_count, degree_mask(classes), C.byref(v)))
        return v.value

    def graph_phase_ms(self) -> dict:
        """device ms of the last graph call's phases while profile_enable() is on: neighbour_reads, lookups, fold"""
        out = np.zeros(3, np.float64)
        self._chk(self.L.brisk_hip_graph_phase_ms(self.h, out))
        return dict(neighbour_reads=float(out[0]), lookups=float(out[1]), fold=float(out[2]))

    # ---- set operations (brisk_hip_merge / intersect / subtract / compare): `other` has the same geometry and is left as it is
    COUNT_RULES = {"left": 0, "min": 1, "max": 2, "sum": 3}

    def merge(self, other: "BriskHip") -> int:
        """self := self UNION other, counts of shared entries added mod 256 -- between saturating indexes min(255, sum), 255 meaning
        "255 or more"; returns the entries new to self.  Both indexes have the same count_mode (EINVAL otherwise)."""
        v = C.c_uint64()
        self._chk(self.L.brisk_hip_merge(self.h, other.h, C.byref(v)))
        return v.value

    def intersect(self, other: "BriskHip", count: str = "left") -> int:
        """keep the entries that are also in `other`; their count is self's ("left"), the "min", the "max" or the "sum"
        (mod 256; between saturating indexes min(255, sum), 255 meaning "255 or more") of the two; returns how many entries were
        removed.  Both indexes have the same count_mode (EINVAL otherwise)."""
        if count not in self.COUNT_RULES:
            raise ValueError(f"count must be one of {sorted(self.COUNT_RULES)}, not {count!r}")
        v = C.c_uint64()
        self._chk(self.L.brisk_hip_intersect(self.h, other.h, self.COUNT_RULES[count], C.byref(v)))
        return v.value

    def subtract(self, other: "BriskHip") -> int:
        """remove the entries that are in `other`, whatever the counts; returns how many were removed"""
        v = C.c_uint64()
        self._chk(self.L.brisk_hip_subtract(self.h, other.h, C.byref(v)))
        return v.value

    def compare(self, other: "BriskHip") -> dict:
        """read-only: entries in both / only here / only there, and over the shared ones the sums of min(count), self's and other's counts"""
        out = np.zeros(6, np.uint64)
        self._chk(self.L.brisk_hip_compare(self.h, other.h, out))
        return dict(zip(("both", "only_self", "only_other", "sum_min", "sum_self", "sum_other"), (int(x) for x in out)))

    def joint_spectrum(self, other: "BriskHip") -> np.ndarray:
        """read-only: uint64[257, 257], J[sa, sb] = identities whose state here is sa and in `other` sb; a state is the stored
        count (0..255) or JOINT_ABSENT = 256, "not in that index" (a wrapped count of 0 is present: state 0).  J[256, 256] is 0.
        Rows 0..255 sum to self.count_spectrum(), columns 0..255 to other's; joint_figures reads completeness and QV off it."""
        out = np.zeros((JOINT_STATES, JOINT_STATES), np.uint64)
        self._chk(self.L.brisk_hip_joint_spectrum(self.h, other.h, out.ctypes.data))
        return out

    def filter_joint(self, other: "BriskHip", min_self: int = 0, max_self: int = 255, min_other: int = 0, max_other: int = 255, keep_absent: bool = False) -> int:
        """keep the entries whose count here is in [min_self, max_self] and whose identity is in `other` with a count in
        [min_other, max_other] -- or, with keep_absent, is not in `other` at all; counts stay; returns how many entries were
        removed.  min_other > max_other: no entry that `other` holds passes (with keep_absent: subtract).  A bound above 255 means 255."""
        bounds = (min_self, max_self, min_other, max_other)
        for v in bounds:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError(f"a count bound must be a non-negative integer, not {v!r}")
        if min_self > max_self:
            raise ValueError("min_self > max_self")
        if min_other > max_other and not keep_absent:
            raise ValueError("nothing can pass: min_other > max_other and keep_absent is false")
        w = _JointWindow(*(min(int(v), 0xffffffff) for v in bounds), 1 if keep_absent else 0, 0)
        v = C.c_uint64()
        self._chk(self.L.brisk_hip_filter_joint(self.h, other.h, C.byref(w), C.byref(v)))
        return v.value

    # ---- snapshots (brisk_hip_save / brisk_hip_load): the index to a file and back, entries as stored
    def save(self, path) -> int:
        """write the index to `path` (whole or not at all: written under a temporary name, then renamed); returns the entries
        written.  The index is left as it was."""
        v = C.c_uint64()
        self._chk(self.L.brisk_hip_save(self.h, os.fsencode(path), C.byref(v)))
        return v.value

    def load(self, path, room: bool = False) -> int:
        """read a snapshot into this EMPTY index of the same layout; returns the entries read.  room=False: compact slices (the
        file's bytes go straight into the arena); room=True: every slice with the room an insert would have given it, for an index
        that keeps growing.  After a failed load the index is empty and usable."""
        v = C.c_uint64()
        self._chk(self.L.brisk_hip_load(self.h, os.fsencode(path), 1 if room else 0, C.byref(v)))
        return v.value

    @classmethod
    def open(cls, path, device: int = 0, room: bool = False, **kw) -> "BriskHip":
        """A new handle with the layout of the snapshot at `path`, and the snapshot loaded into it.  The create options come from
        the header: k, m, b, count_mode and minimizer_mode as stored and part_bits = 0 if ext_bits > 0 else part_bits -- brisk_hip_create extends the routing id
        (ext_bits > 0) only when part_bits was left at its default of 0, and without an extension the stored part_bits is what an
        explicit part_bits gives (min(part_bits, 2b), 2^24 partitions at most by default).  cls_bits also depends on the environment
        (BRISK_CLS_BITS): a file saved under another setting is refused by load (EINVAL, the field named) -- and so is one saved under
        BRISK_CLS_BITS=3 at m = 11, b >= 5 by a library from before such an index had 2^25 partitions (part_bits is named).  **kw: further
        constructor options (max_batch_reads, immediate_inserts, ...)."""
        info = snapshot_info(path)
        kw.setdefault("count_mode", {v: n for n, v in COUNT_MODES.items()}[info["count_mode"]])
        kw.setdefault("minimizer_mode", {v: n for n, v in MINIMIZER_MODES.items()}[info["minimizer_mode"]])
        ix = cls(info["k"], info["m"], info["b"], device=device, part_bits=0 if info["ext_bits"] > 0 else info["part_bits"], **kw)
        try:
            ix.load(path, room=room)
        except Exception:
            ix.close()
            raise
        return ix

    def stats(self) -> dict:
        v = [C.c_uint64() for _ in range(5)]
        self._chk(self.L.brisk_hip_stats(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("nb_buckets", "nb_skmers", "nb_kmers", "memory_bytes", "largest_bucket"), (x.value for x in v)))

    def reallocate_into(self, fresh: "BriskHip") -> None:
        """Brisk::reallocate: move every entry into `fresh`, an empty index over the same k with its own (m, b)."""
        rc = self.L.brisk_hip_reallocate(self.h, fresh.h)
        if rc:
            raise BriskHipError(rc, self.L.brisk_hip_last_error(fresh.h).decode())

    def memory_info(self) -> dict:
        out = np.zeros(4, np.uint64)
        self._chk(self.L.brisk_hip_memory_info(self.h, out))
        return dict(zip(("arena_mapped", "arena_reserved", "pooled", "retired_va"), (int(v) for v in out)))

    def insert_slack(self) -> int:
        """arena entries the single-pass insert reserves beyond a batch's own need (resident insert waves x chunk entries)"""
        v = C.c_uint64()
        self._chk(self.L.brisk_hip_insert_slack(self.h, C.byref(v)))
        return v.value

    def checksum(self) -> tuple:
        """(entries, sum of counts, order-independent digest) of the whole index"""
        out = np.zeros(3, np.uint64)
        self._chk(self.L.brisk_hip_checksum(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def clear(self):
        self._chk(self.L.brisk_hip_clear(self.h))

    def sync(self):
        self._chk(self.L.brisk_hip_sync(self.h))

    # ---- device-buffer paths (pointers are ints: tensor.data_ptr())
    def insert_packed(self, d_packed: int, d_starts: int, n_reads: int):
        self._chk(self.L.brisk_hip_insert_packed(self.h, d_packed, d_starts, n_reads))

    def get_packed(self, d_packed: int, d_starts: int, n_reads: int, d_sums: int):
        """per-read sums of counts (query_sequence), reads and sums on the device"""
        self._chk(self.L.brisk_hip_get_packed(self.h, d_packed, d_starts, n_reads, d_sums))

    def get_kmers_packed(self, d_packed: int, d_starts: int, n_reads: int, d_out: int):
        """per-k-mer answers (brisk_hip_get_kmers), reads and uint16 slots on the device (d_out sized by kmer_slots)"""
        self._chk(self.L.brisk_hip_get_kmers_packed(self.h, d_packed, d_starts, n_reads, d_out))

    def read_profile_packed(self, d_packed: int, d_starts: int, n_reads: int, d_out: int, solid_min: int = 2):
        """per-read abundance records (brisk_hip_read_profile_packed), reads and records (32 bytes a read, READ_PROFILE_DTYPE) on the device"""
        self._chk(self.L.brisk_hip_read_profile_packed(self.h, d_packed, d_starts, n_reads, solid_min, d_out))

    def select_intervals(self, d_profiles: int, n_reads: int, rule: _SelectRule, d_intervals: int):
        """d_intervals[r] (READ_INTERVAL_DTYPE, 8 bytes a read) = the rule applied to d_profiles[r] (brisk_hip_select_intervals), both on
        the device"""
        self._chk(self.L.brisk_hip_select_intervals(self.h, d_profiles, n_reads, C.byref(rule), d_intervals))

    def extract_packed(self, d_packed: int, d_starts: int, n_reads: int, d_intervals: int, d_out_packed: int, out_cap_words: int, d_out_starts: int,
                       d_out_index: Optional[int] = None) -> Tuple[int, int]:
        """the kept intervals of a packed stream as a new packed stream (brisk_hip_extract_packed), everything on the device; returns
        (kept reads, kept nucleotides).  d_out_packed holds out_cap_words >= ceil(nts / 16) + 2 words (as many as the input always do),
        d_out_starts n_reads + 1 uint64, d_out_index (optional) n_reads uint64: the input index of every kept read."""
        n_out, n_nts = C.c_uint64(), C.c_uint64()
        self._chk(self.L.brisk_hip_extract_packed(self.h, d_packed, d_starts, n_reads, d_intervals, d_out_packed, out_cap_words, d_out_starts, d_out_index,
                                                  C.byref(n_out), C.byref(n_nts)))
        return n_out.value, n_nts.value

    def trim_packed(self, d_packed: int, d_starts: int, n_reads: int, d_out_packed: int, out_cap_words: int, d_out_starts: int,
                    d_out_index: Optional[int] = None, solid_min: int = 2, rule: Optional[_SelectRule] = None) -> Tuple[int, int]:
        """read_profile_packed, the rule (default select_rule("solid_run")) and extract_packed in one call (brisk_hip_trim_packed):
        the trimmed or filtered reads as a packed stream that insert_packed, get_packed and read_profile_packed take; returns (kept
        reads, kept nucleotides)"""
        rule = select_rule("solid_run") if rule is None else rule
        n_out, n_nts = C.c_uint64(), C.c_uint64()
        self._chk(self.L.brisk_hip_trim_packed(self.h, d_packed, d_starts, n_reads, solid_min, C.byref(rule), d_out_packed, out_cap_words, d_out_starts, d_out_index,
                                               C.byref(n_out), C.byref(n_nts)))
        return n_out.value, n_nts.value

    def scan_bound(self, d_starts: int, n_reads: int) -> int:
        out = C.c_uint64()
        self._chk(self.L.brisk_hip_scan_bound(self.h, d_starts, n_reads, C.byref(out)))
        return out.value

    def scan_packed(self, d_packed: int, d_starts: int, n_reads: int, d_records: int, cap: int) -> int:
        out = C.c_uint64()
        rc = self.L.brisk_hip_scan_packed(self.h, d_packed, d_starts, n_reads, d_records, cap, C.byref(out))
        if rc == ECAPACITY:
            raise BriskHipError(rc, f"scan needs {out.value} records, cap {cap}")
        self._chk(rc)
        return out.value

    def route_records(self, d_records: int, n: int, d_out: int) -> np.ndarray:
        counts = np.zeros(max(self.layout["n_owners"], 1), np.uint64)
        self._chk(self.L.brisk_hip_route_records(self.h, d_records, n, d_out, counts))
        return counts

    def insert_records(self, d_records: int, n: int):
        self._chk(self.L.brisk_hip_insert_records(self.h, d_records, n))

    def set_owner_cuts(self, first_partition) -> None:
        """owner o holds partitions [first_partition[o], first_partition[o + 1]); the same array on every rank, before anything is routed"""
        cuts = np.ascontiguousarray(first_partition, np.uint64)
        assert len(cuts) == self.layout["n_owners"] + 1
        self._chk(self.L.brisk_hip_set_owner_cuts(self.h, cuts))

    def export_hist(self, d_hist_out: int) -> np.ndarray:
        """copy the last scan's per-partition histogram (2^part_bits u64) to d_hist_out; returns the slice length per owner"""
        lens = np.zeros(max(self.layout["n_owners"], 1), np.uint64)
        self._chk(self.L.brisk_hip_export_hist(self.h, d_hist_out, lens))
        return lens

    def export_hist_add(self, d_hist_acc: int) -> np.ndarray:
        """add the last scan's per-partition histogram to d_hist_acc (2^part_bits u64); returns the slice length per owner"""
        lens = np.zeros(max(self.layout["n_owners"], 1), np.uint64)
        self._chk(self.L.brisk_hip_export_hist_add(self.h, d_hist_acc, lens))
        return lens

    def insert_records_hist(self, d_records: int, n: int, d_hist_slices: int, n_slices: int):
        self._chk(self.L.brisk_hip_insert_records_hist(self.h, d_records, n, d_hist_slices, n_slices))

    def scan_query(self, d_packed: int, d_starts: int, n_reads: int, d_records: int, d_tags: int, cap: int) -> int:
        """query-mode scan: records + the index of the read each came from (u32)"""
        out = C.c_uint64()
        rc = self.L.brisk_hip_scan_query(self.h, d_packed, d_starts, n_reads, d_records, d_tags, cap, C.byref(out))
        if rc == ECAPACITY:
            raise BriskHipError(rc, f"scan needs {out.value} records, cap {cap}")
        self._chk(rc)
        return out.value

    def route_tagged(self, d_records: int, d_tags: int, n: int, d_out: int, d_tags_out: int) -> np.ndarray:
        counts = np.zeros(max(self.layout["n_owners"], 1), np.uint64)
        self._chk(self.L.brisk_hip_route_tagged(self.h, d_records, d_tags, n, d_out, d_tags_out, counts))
        return counts

    def query_records(self, d_records: int, n: int, d_sums: int):
        """d_sums[i] (u64) = sum of the counts of record i's k-mers present in this index"""
        self._chk(self.L.brisk_hip_query_records(self.h, d_records, n, d_sums))

    def scan_kmers(self, d_packed: int, d_starts: int, n_reads: int, d_records: int, d_tags: int, d_anchors: int, cap: int) -> Tuple[int, int]:
        """per-position scan (brisk_hip_scan_kmers): records, a tag each (u32, index into the anchors) and the anchors (u64); returns
        (records, slots of the batch)"""
        n_rec, n_slots = C.c_uint64(), C.c_uint64()
        rc = self.L.brisk_hip_scan_kmers(self.h, d_packed, d_starts, n_reads, d_records, d_tags, d_anchors, cap, C.byref(n_rec), C.byref(n_slots))
        if rc == ECAPACITY:
            raise BriskHipError(rc, f"scan needs {n_rec.value} records, cap {cap}")
        self._chk(rc)
        return n_rec.value, n_slots.value

    def record_kmers(self, d_records: int, n: int, d_offsets: int):
        """d_offsets[0 .. n] (u64) = exclusive prefix sum of the records' k-mer counts (brisk_hip_record_kmers)"""
        self._chk(self.L.brisk_hip_record_kmers(self.h, d_records, n, d_offsets))

    def answer_records(self, d_records: int, n: int, d_offsets: int, d_answers: int):
        """owner side: d_answers[d_offsets[i] + j] (u16) = 0 or 0x100 | count for k-mer j of record i (brisk_hip_answer_records)"""
        self._chk(self.L.brisk_hip_answer_records(self.h, d_records, n, d_offsets, d_answers))

    def place_answers(self, d_records: int, d_tags: int, d_anchors: int, n: int, d_offsets: int, d_answers: int, d_slots: int, n_slots: int):
        """asker side: the answers of the routed records to their slots (brisk_hip_place_answers)"""
        self._chk(self.L.brisk_hip_place_answers(self.h, d_records, d_tags, d_anchors, n, d_offsets, d_answers, d_slots, n_slots))

    def profile_slots(self, d_slots: int, d_starts: int, n_reads: int, d_out: int, solid_min: int = 2):
        """read_profile_packed over slots the caller holds (brisk_hip_profile_slots)"""
        self._chk(self.L.brisk_hip_profile_slots(self.h, d_slots, d_starts, n_reads, solid_min, d_out))

    def _split_call(self, rc: int, st: _SplitStats, raise_on_capacity: bool) -> dict:
        if rc == ECAPACITY and not raise_on_capacity:
            return dict(st.as_dict(), rc=rc)
        self._chk(rc)
        return st.as_dict()

    def solid_runs(self, d_slots: int, d_starts: int, n_reads: int, d_out_frags: int, frag_cap: int, solid_min: int = 2, min_len: int = 0,
                   raise_on_capacity: bool = True) -> dict:
        """The fragment table of slots the caller holds (brisk_hip_solid_runs), everything on the device; fragments_from_slots is the
        definition.  Returns the stats; with raise_on_capacity=False an ECAPACITY answer returns them too, with "rc" set, so that
        the call can be repeated with room.  Needs no index state."""
        st = _SplitStats()
        return self._split_call(self.L.brisk_hip_solid_runs(self.h, d_slots or None, d_starts or None, n_reads, solid_min, min_len, d_out_frags or None, frag_cap, C.byref(st)),
                                st, raise_on_capacity)

    def extract_fragments_packed(self, d_packed: int, d_starts: int, n_reads: int, d_frags: int, n_frags: int, d_out_packed: int, out_cap_words: int, d_out_starts: int) -> int:
        """The rows of a fragment table out of a packed stream, back to back, as a new packed stream (brisk_hip_extract_fragments_packed),
        everything on the device; rows may overlap and repeat a read.  d_out_starts holds n_frags + 1 uint64.  Returns the nucleotides
        written.  Needs no index state."""
        n_nts = C.c_uint64()
        self._chk(self.L.brisk_hip_extract_fragments_packed(self.h, d_packed or None, d_starts or None, n_reads, d_frags or None, n_frags, d_out_packed or None, out_cap_words,
                                                            d_out_starts or None, C.byref(n_nts)))
        return n_nts.value

    def split_packed(self, d_packed: int, d_starts: int, n_reads: int, d_out_packed: int, out_cap_words: int, d_out_starts: int, d_out_frags: int, frag_cap: int,
                     solid_min: int = 2, min_len: int = 0, raise_on_capacity: bool = True) -> dict:
        """The per-k-mer lookups, the runs and the gather in one call (brisk_hip_split_packed): the fragments of a packed stream as a
        packed stream that insert_packed, get_packed and read_profile_packed take; d_out_packed (with out_cap_words 0) and d_out_frags
        may be 0.  Returns the stats, as solid_runs does."""
        st = _SplitStats()
        return self._split_call(self.L.brisk_hip_split_packed(self.h, d_packed or None, d_starts or None, n_reads, solid_min, min_len, d_out_packed or None, out_cap_words,
                                                              d_out_starts or None, d_out_frags or None, frag_cap, C.byref(st)), st, raise_on_capacity)

    def _correct_call(self, rc: int, st: _CorrectStats, raise_on_capacity: bool) -> dict:
        if rc == ECAPACITY and not raise_on_capacity:
            return dict(st.as_dict(), rc=rc)
        self._chk(rc)
        return st.as_dict()

    def weak_sites(self, d_slots: int, d_starts: int, n_reads: int, d_out_sites: int, site_cap: int, solid_min: int = 2, min_cover: Optional[int] = None,
                   raise_on_capacity: bool = True) -> dict:
        """The site table of slots the caller holds (brisk_hip_weak_sites), everything on the device; sites_from_slots is the
        definition.  Returns the stats; with raise_on_capacity=False an ECAPACITY answer returns them too, with "rc" set.  Needs
        no index state."""
        st = _CorrectStats()
        return self._correct_call(self.L.brisk_hip_weak_sites(self.h, d_slots or None, d_starts or None, n_reads, solid_min, int(min_cover or 0), d_out_sites or None, site_cap,
                                                              C.byref(st)), st, raise_on_capacity)

    def candidate_windows(self, d_packed: int, d_starts: int, n_reads: int, d_sites: int, n_sites: int, d_out_packed: int, out_cap_words: int, d_out_starts: int) -> int:
        """The 3 * n_sites candidate windows of a site table as a packed stream, substituted (brisk_hip_candidate_windows), everything
        on the device.  d_out_starts holds 3 * n_sites + 1 uint64.  Returns the nucleotides written.  Needs no index state."""
        n_nts = C.c_uint64()
        self._chk(self.L.brisk_hip_candidate_windows(self.h, d_packed or None, d_starts or None, n_reads, d_sites or None, n_sites, d_out_packed or None, out_cap_words,
                                                     d_out_starts or None, C.byref(n_nts)))
        return n_nts.value

    def decide_sites(self, d_cand_slots: int, d_sites: int, n_sites: int, d_packed: int, d_starts: int, n_reads: int, d_out_corrections: int, corr_cap: int,
                     solid_min: int = 2, raise_on_capacity: bool = True) -> dict:
        """Candidate slots to correction rows (brisk_hip_decide_sites), everything on the device; corrections_from_candidates is the
        definition.  Returns the stats (n_sites and the three decision counters).  Needs no index state."""
        st = _CorrectStats()
        return self._correct_call(self.L.brisk_hip_decide_sites(self.h, d_cand_slots or None, d_sites or None, n_sites, d_packed or None, d_starts or None, n_reads, solid_min,
                                                                d_out_corrections or None, corr_cap, C.byref(st)), st, raise_on_capacity)

    def apply_corrections(self, d_packed: int, d_starts: int, n_reads: int, d_corr: int, n_corr: int, d_out_packed: int, out_cap_words: int):
        """The patched copy of a packed stream (brisk_hip_apply_corrections), everything on the device.  Needs no index state."""
        self._chk(self.L.brisk_hip_apply_corrections(self.h, d_packed or None, d_starts or None, n_reads, d_corr or None, n_corr, d_out_packed or None, out_cap_words))

    def correct_packed(self, d_packed: int, d_starts: int, n_reads: int, d_out_packed: int, out_cap_words: int, d_out_corrections: int, corr_cap: int,
                       solid_min: int = 2, min_cover: Optional[int] = None, raise_on_capacity: bool = True) -> dict:
        """Lookups, sites, candidates, decisions and the patched copy in one call (brisk_hip_correct_packed): the corrected stream
        has the input's read table and goes straight to insert_packed, get_packed or read_profile_packed; d_out_packed (with
        out_cap_words 0) and d_out_corrections (with corr_cap 0) may be 0.  Returns the stats, as weak_sites does."""
        st = _CorrectStats()
        return self._correct_call(self.L.brisk_hip_correct_packed(self.h, d_packed or None, d_starts or None, n_reads, solid_min, int(min_cover or 0), d_out_packed or None,
                                                                  out_cap_words, d_out_corrections or None, corr_cap, C.byref(st)), st, raise_on_capacity)

    def pack_ascii(self, d_bases: int, n_bases: int, d_packed: int):
        self._chk(self.L.brisk_hip_pack_ascii(self.h, d_bases, n_bases, d_packed))

    def intake_ascii(self, d_bases: int, d_quals: int, d_offsets: int, n_reads: int, rule: _IntakeRule, d_out_packed: int, out_cap_words: int,
                     d_out_starts: int, d_out_frags: int, frag_cap: int, raise_on_capacity: bool = True) -> dict:
        """Raw bytes on the device -> fragments as a packed stream (brisk_hip_intake_ascii); d_quals, d_out_packed (with out_cap_words
        0) and d_out_frags may be 0.  Returns the stats; with raise_on_capacity=False an ECAPACITY answer returns them too, with
        "rc" set, so that the call can be repeated with room."""
        st = _IntakeStats()
        rc = self.L.brisk_hip_intake_ascii(self.h, d_bases or None, d_quals or None, d_offsets or None, n_reads, C.byref(rule) if rule is not None else None,
                                           d_out_packed or None, out_cap_words, d_out_starts or None, d_out_frags or None, frag_cap, C.byref(st))
        if rc == ECAPACITY and not raise_on_capacity:
            return dict(st.as_dict(), rc=rc)
        self._chk(rc)
        return st.as_dict()

    def fragment_intervals(self, d_frags: int, n_frags: int, n_reads: int, d_intervals: int):
        """d_intervals[r] = the first longest fragment of read r in an intake fragment table (brisk_hip_fragment_intervals), both on
        the device; intervals_from_fragments is the definition"""
        self._chk(self.L.brisk_hip_fragment_intervals(self.h, d_frags or None, n_frags, n_reads, d_intervals or None))

    def pair_intervals(self, d_each: int, d_whole: Optional[int], n_reads: int, pair_mode, d_out: int):
        """the pair decision over interleaved intervals on the device (brisk_hip_pair_intervals); d_out may be d_each; the module's
        pair_intervals is the definition"""
        self._chk(self.L.brisk_hip_pair_intervals(self.h, d_each or None, d_whole or None, n_reads, pair_mode if isinstance(pair_mode, int) else _pair_mode(pair_mode), d_out or None))

    def compose_intervals(self, d_outer: int, n_reads: int, d_inner: int, d_index: int, n_kept: int, d_out: int):
        """two cuts chained on the device (brisk_hip_compose_intervals); the module's compose_intervals is the definition"""
        self._chk(self.L.brisk_hip_compose_intervals(self.h, d_outer or None, n_reads, d_inner or None, d_index or None, n_kept, d_out or None))

    def _pairs_call(self, rc: int, pc: _PairCounts, raise_on_capacity: bool) -> dict:
        if rc == ECAPACITY and not raise_on_capacity:
            return dict(pc.as_dict(), rc=rc)
        self._chk(rc)
        return pc.as_dict()

    def extract_pairs_packed(self, d_packed: int, d_starts: int, n_reads: int, d_intervals: int, pairs, singles=None, raise_on_capacity: bool = True) -> dict:
        """An interleaved packed stream split into intact pairs and singles (brisk_hip_extract_pairs_packed), everything on the device.
        pairs / singles: (d_out_packed, out_cap_words, d_out_starts, d_out_index) as extract_packed takes them; singles None: counted
        and dropped.  Returns the counts (PAIR_COUNTS_FIELDS); with raise_on_capacity=False an ECAPACITY answer returns them too, with
        "rc" set, so that the call can be repeated with room."""
        pc = _PairCounts()
        p, s = _pair_out(pairs), _pair_out(singles)
        return self._pairs_call(self.L.brisk_hip_extract_pairs_packed(self.h, d_packed or None, d_starts or None, n_reads, d_intervals or None, *p, *s, C.byref(pc)), pc, raise_on_capacity)

    def trim_pairs_packed(self, d_packed: int, d_starts: int, n_reads: int, pairs, singles=None, solid_min: int = 2, rule: Optional[_SelectRule] = None, pair_mode="each",
                          raise_on_capacity: bool = True) -> dict:
        """trim_packed for clean interleaved reads (brisk_hip_trim_pairs_packed): profile, rule, pair decision, pairs and singles as
        two packed streams; arguments and result as extract_pairs_packed"""
        rule = select_rule("solid_run") if rule is None else rule
        pc = _PairCounts()
        p, s = _pair_out(pairs), _pair_out(singles)
        return self._pairs_call(self.L.brisk_hip_trim_pairs_packed(self.h, d_packed or None, d_starts or None, n_reads, solid_min, C.byref(rule), _pair_mode(pair_mode), *p, *s, C.byref(pc)),
                                pc, raise_on_capacity)

    def clean_pairs_ascii(self, d_bases: int, d_quals: int, d_offsets: int, n_reads: int, intake: _IntakeRule, pairs, singles=None, rule: Optional[_SelectRule] = None,
                          solid_min: int = 2, pair_mode="each", d_out_intervals: int = 0, raise_on_capacity: bool = True):
        """Raw interleaved bytes on the device to clean pairs and singles (brisk_hip_clean_pairs_ascii); returns (counts, intake stats)"""
        pc, st = _PairCounts(), _IntakeStats()
        p, s = _pair_out(pairs), _pair_out(singles)
        rc = self.L.brisk_hip_clean_pairs_ascii(self.h, d_bases or None, d_quals or None, d_offsets or None, n_reads, C.byref(intake) if intake is not None else None,
                                                C.byref(rule) if rule is not None else None, solid_min, _pair_mode(pair_mode), *p, *s, d_out_intervals or None, C.byref(pc), C.byref(st))
        return self._pairs_call(rc, pc, raise_on_capacity), st.as_dict()

    def unpack_ascii(self, d_packed: int, first_nt: int, n_nts: int, d_bases: int):
        """d_bases[i] = "ACTG"[code of nucleotide first_nt + i of the packed stream] (brisk_hip_unpack_ascii): pack_ascii's inverse"""
        self._chk(self.L.brisk_hip_unpack_ascii(self.h, d_packed, first_nt, n_nts, d_bases))

    def synth_reads(self, genome_len: int, first_read: int, n_reads: int, read_len: int, d_packed: int, d_starts: int,
                    seed_g: int = 1, seed_r: int = 2):
        self._chk(self.L.brisk_hip_synth_reads(self.h, genome_len, first_read, n_reads, read_len, seed_g, seed_r, d_packed, d_starts))

    # ---- per-call API (entry-id mode), as the C++ facade uses it
    def scan_sequence(self, seq):
        s = seq.encode() if isinstance(seq, str) else bytes(seq)
        nk = max(len(s) - self.k + 1, 1)
        ret = np.zeros(nk, np.uint64); cnt = np.zeros(nk, np.uint32)
        lo = np.zeros(nk, np.uint64); hi = np.zeros(nk, np.uint64); idx = np.zeros(nk, np.uint8)
        n = C.c_uint64()
        self._chk(self.L.brisk_hip_scan_sequence(self.h, s, len(s), nk, ret, cnt, lo, hi, idx, C.byref(n)))
        t = int(cnt[: n.value].sum())
        return ret[: n.value], cnt[: n.value], lo[:t], hi[:t], idx[:t]

    def upsert_kmers(self, lo, hi, idx):
        lo = np.ascontiguousarray(lo, np.uint64); hi = np.ascontiguousarray(hi, np.uint64); idx = np.ascontiguousarray(idx, np.uint8)
        ids = np.zeros(max(len(lo), 1), np.uint32); new = np.zeros(max(len(lo), 1), np.uint8)
        self._chk(self.L.brisk_hip_upsert_kmers(self.h, lo, hi, idx, len(lo), ids, new))
        return ids[: len(lo)], new[: len(lo)]

    def find_kmers(self, lo, hi, idx):
        lo = np.ascontiguousarray(lo, np.uint64); hi = np.ascontiguousarray(hi, np.uint64); idx = np.ascontiguousarray(idx, np.uint8)
        ids = np.zeros(max(len(lo), 1), np.uint32)
        self._chk(self.L.brisk_hip_find_kmers(self.h, lo, hi, idx, len(lo), ids))
        return ids[: len(lo)]

    def enumerate_ids(self, chunk: int = 1 << 20):
        cur = C.c_uint64(0); n = C.c_uint64(0)
        out = [[], [], [], []]
        cap = chunk
        while True:
            lo = np.zeros(cap, np.uint64); hi = np.zeros(cap, np.uint64); idx = np.zeros(cap, np.uint8); ids = np.zeros(cap, np.uint32)
            rc = self.L.brisk_hip_enumerate_ids(self.h, C.byref(cur), lo, hi, idx, ids, cap, C.byref(n))
            if rc == ECAPACITY:
                cap *= 4
                continue
            self._chk(rc)
            if n.value == 0:
                break
            for a, v in zip(out, (lo, hi, idx, ids)):
                a.append(v[: n.value])
        dts = (np.uint64, np.uint64, np.uint8, np.uint32)
        return tuple(np.concatenate(a) if a else np.zeros(0, dt) for a, dt in zip(out, dts))

    def debug_order_keys(self, mmers, exact: bool = False) -> np.ndarray:
        x = np.ascontiguousarray(mmers, np.uint64)
        out = np.zeros(max(len(x), 1), np.uint64)
        self._chk(self.L.brisk_hip_debug_order_keys(self.h, x, len(x), 1 if exact else 0, out))
        return out[: len(x)]

    def debug_guard_count(self) -> int:
        """Keys of the last debug_order_keys call whose class sums lay in the guard band (decided by the exact fold)."""
        n = C.c_uint64(0)
        self.L.brisk_hip_debug_guard_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]  # (bound on use: a test hook, not part of load())
        self._chk(self.L.brisk_hip_debug_guard_count(self.h, C.byref(n)))
        return int(n.value)

    def debug_touched(self) -> np.ndarray:
        """The partitions the last record insert touched, in the order its insert kernels walked them (a test hook)."""
        f = self.L.brisk_hip_debug_touched  # (bound on use: a test hook, not part of load())
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        n = C.c_uint64(0)
        self._chk(f(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(int(n.value), 1), np.uint32)
        self._chk(f(self.h, out.ctypes.data, len(out), C.byref(n)))
        return out[: int(n.value)]

    def debug_directory(self, parts):
        """(entries in use, slice capacity) of the given partitions, two uint32 arrays (a test hook)."""
        f = self.L.brisk_hip_debug_directory  # (bound on use)
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        p = np.ascontiguousarray(parts, np.uint32)
        cnt, cap = np.zeros(max(len(p), 1), np.uint32), np.zeros(max(len(p), 1), np.uint32)
        self._chk(f(self.h, p.ctypes.data, len(p), cnt.ctypes.data, cap.ctypes.data))
        return cnt[: len(p)], cap[: len(p)]

    # ---- measurement
    def profile_enable(self, on: bool = True):
        self._chk(self.L.brisk_hip_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        self._chk(self.L.brisk_hip_profile_reset(self.h))

    def profile_read(self) -> dict:
        n = C.c_uint32()
        names = (C.c_char_p * 16)()
        launches = (C.c_uint64 * 16)()
        ms = (C.c_double * 16)()
        self._chk(self.L.brisk_hip_profile_read(self.h, C.byref(n), names, launches, ms))
        return {names[i].decode(): {"launches": launches[i], "ms": ms[i]} for i in range(n.value)}
