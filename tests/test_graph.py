"""GPU: de Bruijn adjacency (brisk_hip_adjacency / _degree_spectrum / _prune_degrees).  The cases run once, in a child
process (tests/graph_worker.py), and every test here reads its own case's verdict:

1. composition: adjacency(mc) = adjacency_from_slots(get_kmers(neighbour_strings(enumerate()))), byte for byte, at every geometry and
   min_count 0, 1, 2, 255; in both count modes; on homopolymers and periodic reads; on a reference-mode k63 index;
2. truth: on tie-free reads, bit j is set exactly when the canonical form of neighbour string j is in a Python dictionary of the reads'
   canonical k-mers with multiplicity >= min_count;
3. crafted graphs through degree_spectrum and graph_figures: a path, a fork, an isolated node, a ring, a thresholded path;
4. adjacency_device into a caller's buffer, ECAPACITY with the buffer untouched, degree_spectrum against the host fold, the sum;
5. rounds: children under BRISK_GRAPH_BATCH = 1 and 5 give the bytes of the default, on a directory with a partition of more than 64
   entries and empty partitions between non-empty ones;
6. prune_degrees: rows, digest against an index built afresh, lookups, re-insert, snapshot semantics, empty mask and empty window;
7. refusals by code and message; 8. brisk_count --degrees / --prune-degrees."""
import json
import os
import subprocess
import sys

import pytest

from graph_worker import GEOMETRIES, name_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "graph_worker.py")
_verdicts = {}


def passed(name, tmp_path_factory):
    """the worker's verdict on one case: all cases run in one child, once"""
    if not _verdicts:
        out = str(tmp_path_factory.mktemp("graph") / "verdicts.json")
        p = subprocess.run([sys.executable, WORKER, out], capture_output=True, text=True, timeout=900)
        if os.path.exists(out):
            with open(out) as f:
                _verdicts.update(json.load(f))
        _verdicts["<worker>"] = "ok" if p.returncode == 0 and "done" in p.stdout else "exit %s\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
        print(p.stdout)
    assert _verdicts["<worker>"] == "ok", _verdicts["<worker>"]
    v = _verdicts[name]
    print(name, v)
    assert v.startswith("ok"), v


@pytest.mark.parametrize("k,m,b,mode", GEOMETRIES)
def test_adjacency_is_the_composition_of_the_public_calls(k, m, b, mode, tmp_path_factory):
    passed("composition-" + name_of(k, m, b, mode), tmp_path_factory)


def test_composition_in_both_count_modes(tmp_path_factory):
    passed("composition-count_modes", tmp_path_factory)


def test_composition_where_ties_abound(tmp_path_factory):
    passed("composition-ties", tmp_path_factory)


def test_composition_on_a_reference_mode_k63_index(tmp_path_factory):
    passed("composition-reference_k63", tmp_path_factory)


@pytest.mark.parametrize("k,m,b,mode", GEOMETRIES)
def test_adjacency_is_the_truth_on_tie_free_reads(k, m, b, mode, tmp_path_factory):
    passed("truth-" + name_of(k, m, b, mode), tmp_path_factory)


def test_crafted_graphs(tmp_path_factory):
    passed("crafted", tmp_path_factory)


def test_device_and_host_forms(tmp_path_factory):
    passed("forms", tmp_path_factory)


def test_rounds_do_not_change_the_bytes(tmp_path_factory):
    passed("rounds", tmp_path_factory)


@pytest.mark.parametrize("k,m,b,mode", [GEOMETRIES[0], GEOMETRIES[2], GEOMETRIES[3]])
def test_prune_degrees(k, m, b, mode, tmp_path_factory):
    passed("prune_degrees-" + name_of(k, m, b, mode), tmp_path_factory)


def test_refusals(tmp_path_factory):
    passed("refusals", tmp_path_factory)


def test_brisk_count_degrees_and_prune_degrees(tmp_path_factory):
    passed("brisk_count", tmp_path_factory)
