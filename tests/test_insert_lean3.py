"""GPU: the third instance slot of k_insert_first (DESIGN.md section 4 finding 16), pinned where it begins and ends.

k_insert_first takes an empty partition of at most 64 records and at most 192 k-mer instances after the containment fold.  The
read sets (tests/insert_lean3_reads.py) hold a few dozen partitions each of exactly 128, 129, 191, 192 and 193 distinct k-mers
at k63 m21 b14, set one with every k-mer once, set two with contained records on them; tests/test_insert_lean3_cpu.py shows on
the CPU that they are what is claimed here.  The worker (one child process per environment) compares every index with the
oracle's: full enumeration, nb_kmers, nb_buckets, digest.  This file asserts the route from the library's `path:` lines:

    OVER <= left over <= OVER + AMBIG        (the oracle's per-partition numbers: insert_lean3_reads.census)

and AMBIG < S3, so a kernel that left the partitions of 129 .. 192 instances over would fail the right-hand side."""
import json
import os
import re
import subprocess
import sys

import pytest

import oracle
import insert_lean3_reads as R

pytestmark = pytest.mark.gpu

LEAN = re.compile(r"insert of (\d+) records \((\w+) layout.* into (\d+) partitions: k_insert_first \(fresh index\): (\d+) partitions lean, (\d+) left over to k_insert, "
                  r"(\d+) partitions to k_insert_huge")
GENERAL = re.compile(r"insert of (\d+) records \((\w+) layout.* into (\d+) partitions: k_insert, (\d+) partitions to k_insert_huge")
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "insert_lean3_worker.py")
_runs = {}


def run(scenario, **env_add):
    key = (scenario, tuple(sorted(env_add.items())))
    if key in _runs:
        return _runs[key]
    env = {k: v for k, v in os.environ.items() if not k.startswith("BRISK_") or k == "BRISK_HIP_LIB"}
    env.update(BRISK_TRACE="1", **env_add)
    p = subprocess.run([sys.executable, WORKER, scenario], env=env, capture_output=True, text=True, timeout=600)
    stages, name = {}, "start"
    for line in p.stderr.splitlines():
        if line.startswith("[lean] stage "):
            name = line.split()[-1]
        elif line.startswith("[brisk_hip]") and "path: insert of" in line:
            stages.setdefault(name, []).append(line)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (scenario, env_add, p.stdout[-3000:], p.stderr[-6000:])
    results = {}
    for line in p.stdout.splitlines():
        k, _, v = line.partition(" ")
        if v:
            results[k] = json.loads(v)
    _runs[key] = (stages, results)
    return _runs[key]


@pytest.fixture(scope="module")
def censuses():
    oracle.build(ref=False)
    O = oracle.Oracle()
    return {"one": R.census(O, R.set_one()), "two": R.census(O, R.set_two())}


def lean_line(stages, name):
    lines = stages.get(name, [])
    assert len(lines) == 1, (name, stages)
    m = LEAN.search(lines[0])
    assert m, lines
    rec, layout, touched, lean, left, huge = m.groups()
    assert int(lean) + int(left) + int(huge) == int(touched), lines
    return {"touched": int(touched), "lean": int(lean), "left": int(left), "huge": int(huge)}


@pytest.mark.parametrize("which", ["one", "two"])
def test_partitions_of_129_to_192_instances_go_lean(censuses, which):
    stages, results = run("main")
    c, r = censuses[which], lean_line(stages, which)
    print(which, r, c)
    assert c["AMBIG"] < c["S3"], c
    assert r["touched"] == c["partitions"] and r["huge"] == 0, (r, c)
    assert c["OVER"] <= r["left"] <= c["OVER"] + c["AMBIG"], (r, c)


@pytest.mark.parametrize("which", ["one", "two"])
def test_same_index_with_the_lean_route_switched_off(which):
    stages, results = run("main")
    off_stages, off = run("first-batches", BRISK_INSERT_LEAN="0")
    lines = off_stages.get(which, [])
    assert len(lines) == 1 and GENERAL.search(lines[0]) and "k_insert_first" not in lines[0], lines
    assert off[which] == results[which]  # entries, sum of counts, digest (each equal to the oracle's: the worker)


def test_second_batch_takes_the_general_route():
    stages, results = run("main")
    lean_line(stages, "one-again")
    lines = stages.get("second", [])
    assert len(lines) == 1 and GENERAL.search(lines[0]) and "k_insert_first" not in lines[0], lines


def test_saturating_index(censuses):
    stages, results = run("main")
    r, c = lean_line(stages, "sat-one"), censuses["one"]
    assert c["OVER"] <= r["left"] <= c["OVER"] + c["AMBIG"], (r, c)  # the saturating instantiation, the same route
    assert lean_line(stages, "sat-hot")["lean"] > 0  # (counts of 255 for the copy read 300 times: checked in the worker)
