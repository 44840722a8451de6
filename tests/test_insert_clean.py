"""GPU: the table-free path of k_insert_first (DESIGN.md section 4 finding 19).

Where the containment fold proves that no two k-mer instances of a partition are equal, k_insert_first stores instance i as entry i
and leaves the probe table out.  The read sets (tests/insert_clean_reads.py) are crafted partitions at k63 m21 b14: clean ones of
exactly 64, 65, 128, 129 and 192 instances, without and with records that fold, two loci of one bucket, and partitions the table
must take (partial overlaps of one locus, a chain of them, a record overlapped from both sides, a substitution outside the core,
more heads than the fold takes); tests/test_insert_clean_cpu.py shows on the CPU that they are what is claimed here.  The worker
(one child process per environment) compares every index with the oracle's: full enumeration, nb_kmers, nb_buckets, digest.
This file asserts the route from the library's `path:` lines:

    CLEAN <= table-free <= CLEAN + AMBIG        (the fold's rules over the oracle's records: insert_clean_reads.census)

and with BRISK_INSERT_CLEAN=0 the same indexes with 0 table-free."""
import json
import os
import re
import subprocess
import sys

import pytest

import oracle
import insert_clean_reads as R

pytestmark = pytest.mark.gpu

LEAN = re.compile(r"insert of (\d+) records \((\w+) layout.* into (\d+) partitions: k_insert_first \(fresh index\): (\d+) partitions lean, (\d+) left over to k_insert, "
                  r"(\d+) partitions to k_insert_huge \((\d+) table-free\)$")
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "insert_clean_worker.py")
_runs = {}


def run(**env_add):
    key = tuple(sorted(env_add.items()))
    if key in _runs:
        return _runs[key]
    env = {k: v for k, v in os.environ.items() if not k.startswith("BRISK_") or k == "BRISK_HIP_LIB"}
    env.update(BRISK_TRACE="1", **env_add)
    p = subprocess.run([sys.executable, WORKER], env=env, capture_output=True, text=True, timeout=600)
    stages, name = {}, "start"
    for line in p.stderr.splitlines():
        if line.startswith("[lean] stage "):
            name = line.split()[-1]
        elif line.startswith("[brisk_hip]") and "path: insert of" in line:
            stages.setdefault(name, []).append(line)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (env_add, p.stdout[-3000:], p.stderr[-6000:])
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
    c = {name: R.census(O, R.get(name)) for name in R.SETS}
    c["hot"] = R.census(O, R._pack(R.hot_reads(300)))
    return c


def path_line(stages, name):
    lines = stages.get(name, [])
    assert len(lines) == 1, (name, stages)
    m = LEAN.search(lines[0])
    assert m, lines
    rec, layout, touched, lean, left, huge, free = m.groups()
    assert int(lean) + int(left) + int(huge) == int(touched), lines
    return {"touched": int(touched), "lean": int(lean), "left": int(left), "huge": int(huge), "free": int(free)}


@pytest.mark.parametrize("name", R.SETS)
def test_clean_partitions_go_table_free_and_no_others(censuses, name):
    stages, results = run()
    c, r = censuses[name], path_line(stages, name)
    print(name, r, {k: v for k, v in c.items() if k != "states"})
    assert c["AMBIG"] < c["CLEAN"] or c["CLEAN"] == 0, c
    assert r["touched"] == c["partitions"] and r["lean"] == c["LEAN"] and r["huge"] == 0, (r, c)
    assert c["CLEAN"] <= r["free"] <= c["CLEAN"] + c["AMBIG"], (r, c)


@pytest.mark.parametrize("name", ["folds", "mixed"])
def test_saturating_index(censuses, name):
    stages, results = run()
    c, r = censuses[name], path_line(stages, "sat-" + name)
    assert c["CLEAN"] <= r["free"] <= c["CLEAN"] + c["AMBIG"] and r["lean"] == c["LEAN"], (r, c)
    assert results["sat-" + name] == results[name]  # (no count near 255: the same entries, counts and digest)


def test_a_read_300_times_over_a_clean_partition(censuses):
    stages, results = run()
    c, r = censuses["hot"], path_line(stages, "sat-hot")  # (counts of 255: checked in the worker)
    assert (r["touched"], r["left"], r["lean"], r["free"]) == (c["partitions"], 1, c["LEAN"], c["CLEAN"]), (r, c)


@pytest.mark.parametrize("name", R.SETS + ("sat-folds", "sat-mixed", "sat-hot"))
def test_same_index_with_the_table_free_path_switched_off(name):
    stages, results = run()
    off_stages, off = run(BRISK_INSERT_CLEAN="0")
    on, r = path_line(stages, name), path_line(off_stages, name)
    assert r["free"] == 0 and (r["touched"], r["lean"], r["left"]) == (on["touched"], on["lean"], on["left"]), (r, on)
    assert off[name] == results[name]  # entries, sum of counts, digest (each equal to the oracle's: the worker)
