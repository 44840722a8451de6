"""brisk_amd -- MI355X-native Brisk hot path.

The product is ``libbrisk_hip.so`` (HIP kernels + the C-ABI of
``include/brisk_hip.h``) and the C++ facade in ``brisk_amd/include``.  This
Python package is a thin ctypes view of the C-ABI used by tests, ``bench.py``
and ``__graft_entry__``; it never computes anything itself and raises if the
library is missing (there is no CPU fallback).
"""
from .hipapi import BriskHip, BriskHipError, build_apps, build_library, library_path, coef_table, kmer_slots, snapshot_info, READ_PROFILE_DTYPE, profile_from_slots, COUNT_MODES, MINIMIZER_MODES  # noqa: F401
from .hipapi import READ_INTERVAL_DTYPE, SELECT_KINDS, intervals_from_profile, select_rule  # noqa: F401
from .hipapi import JOINT_ABSENT, joint_figures, joint_spectrum_from_entries  # noqa: F401
from .hipapi import DEGREE_CLASSES, adjacency_from_slots, degree_class, degree_mask, degree_spectrum_from_adjacency, graph_figures, neighbour_strings  # noqa: F401
from .hipapi import FRAGMENT_DTYPE, INTAKE_BLOCK, INTAKE_STATS_FIELDS, fragments_from_reads, intake_rule  # noqa: F401
from .hipapi import PAIR_COUNTS_FIELDS, PAIR_MODES, compose_intervals, intervals_from_fragments, pair_intervals, split_pairs  # noqa: F401
from .hipapi import SPLIT_STATS_FIELDS, fragments_from_slots  # noqa: F401
from .hipapi import CORRECT_STATS_FIELDS, CORRECTION_DTYPE, SITE_DTYPE, corrections_from_candidates, site_windows, sites_from_slots  # noqa: F401
