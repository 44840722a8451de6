"""GPU: full-width minimizers (brisk_hip_options.minimizer_mode = BRISK_HIP_MINIMIZER_FULL).  The cases run once, in a child process
(tests/minimizer_mode_worker.py), each against the Python restatement of the enumerator (tests/minimizer_reference.py) or a host
set -- never against the library -- and every test here reads its own case's verdict:

1. parity: enumerate() of a full-mode index = index_of(reads, full=True) as a multiset with counts, at every geometry, on random,
   periodic and homopolymer reads of k, k + 1, 2k - 1 and 150 nt and sequences long enough to be scanned in chunks, each inserted
   twice; the same in reference mode as a control of the harness.  Only the full-mode cases at k > 32 can fail without the feature;
2. k <= 32: both modes build the same index (checksum) at k31 m15 and k31 m11;
3. one k-mer, one entry: on a tie-free input at k63 m21 the entries are the host's distinct canonical k-mers and the count spectrum
   the histogram of their multiplicities; the reference-mode index of the same reads has more entries;
4. strand: the reverse complements build the same index, and find every slot of the forward index;
5. windows: every 2k - 1 window of 400 reads, looked up as a read of its own, is found whole (DESIGN.md section 4.k's experiment);
6. correction: on planted substitutions every correction made on the full-mode index is the planted truth, and there are at least as
   many as on the reference-mode index;
7. plumbing: layout, save / open / load, mixed modes refused by name, reallocate, brisk_hip_scan_sequence, brisk_count;
8. sharded: two owners on one device add up to the single index."""
import json
import os
import subprocess
import sys

import pytest

from minimizer_mode_worker import GEOMETRIES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "minimizer_mode_worker.py")
_verdicts = {}


def verdict(name, tmp_path_factory):
    """the worker's verdict on one case: all cases run in one child, once"""
    if not _verdicts:
        out = str(tmp_path_factory.mktemp("minimizer_mode") / "verdicts.json")
        p = subprocess.run([sys.executable, WORKER, out], capture_output=True, text=True, timeout=1200)
        if os.path.exists(out):
            with open(out) as f:
                _verdicts.update(json.load(f))
        _verdicts["<worker>"] = "ok" if p.returncode == 0 and "done" in p.stdout else "exit %s\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
        print(p.stdout)
    assert _verdicts["<worker>"] == "ok", _verdicts["<worker>"]
    return _verdicts[name]


def passed(name, tmp_path_factory):
    v = verdict(name, tmp_path_factory)
    print(name, v)
    assert v.startswith("ok"), v


@pytest.mark.parametrize("mode", ("full", "reference"))
@pytest.mark.parametrize("k,m,b", GEOMETRIES)
def test_parity_with_the_restatement(k, m, b, mode, tmp_path_factory):
    passed("parity-k%d-m%d-b%d-%s" % (k, m, b, mode), tmp_path_factory)


def test_both_modes_build_the_same_index_up_to_k32(tmp_path_factory):
    passed("k_up_to_32", tmp_path_factory)


def test_one_kmer_one_entry(tmp_path_factory):
    passed("one_entry", tmp_path_factory)


def test_the_reverse_complements_build_and_find_the_same_index(tmp_path_factory):
    passed("strand", tmp_path_factory)


def test_every_window_is_found_whole(tmp_path_factory):
    passed("windows", tmp_path_factory)


def test_corrections_on_a_full_mode_index_are_the_planted_truth(tmp_path_factory):
    """On the planted-substitution input of test_correct.py's k31 case, moved to k63 m21 with min_cover = k.  The numbers of
    corrections on both indexes are in the verdict's text (the test's output)."""
    passed("correction", tmp_path_factory)


def test_the_mode_travels_and_is_checked(tmp_path_factory):
    passed("plumbing", tmp_path_factory)


def test_two_owners_add_up_to_the_single_index(tmp_path_factory):
    passed("sharded", tmp_path_factory)
