"""GPU: the grouped fold of k_insert_first (DESIGN.md section 4 finding 21).

k_insert_first takes the fold head of every core-key group in the same round (fold_records_grouped) and hands a partition to the
sequential fold where more than 16 heads were taken.  The read sets (tests/insert_fold_groups_worker.py) are crafted partitions at the
smallest shapes at which the slot logic, the round bound and the fallback can go wrong; tests/test_fold_groups_cpu.py shows on the
CPU that they are what is claimed.  The worker (one child process) compares every index, plain and saturating, with the oracle's:
full enumeration, nb_kmers, nb_buckets, digest.  This file asserts the route from the library's `path:` lines against the census
of both restated rules (fold_group_rules) and against insert_clean_reads.census: partitions touched, lean, left over, table-free."""
import json
import os
import re
import subprocess
import sys

import pytest

import oracle
import insert_clean_reads as R
import insert_fold_groups_worker as W

pytestmark = pytest.mark.gpu

LEAN = re.compile(r"insert of (\d+) records \((\w+) layout.* into (\d+) partitions: k_insert_first \(fresh index\): (\d+) partitions lean, (\d+) left over to k_insert, "
                  r"(\d+) partitions to k_insert_huge \((\d+) table-free\)$")

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "insert_fold_groups_worker.py")
_run = []


def run():
    if not _run:
        env = {k: v for k, v in os.environ.items() if not k.startswith("BRISK_") or k == "BRISK_HIP_LIB"}
        env.update(BRISK_TRACE="1")
        p = subprocess.run([sys.executable, WORKER], env=env, capture_output=True, text=True, timeout=600)
        stages, name = {}, "start"
        for line in p.stderr.splitlines():
            if line.startswith("[lean] stage "):
                name = line.split()[-1]
            elif line.startswith("[brisk_hip]") and "path: insert of" in line:
                stages.setdefault(name, []).append(line)
        assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout[-3000:], p.stderr[-6000:])
        results = {}
        for line in p.stdout.splitlines():
            k, _, v = line.partition(" ")
            if v:
                results[k] = json.loads(v)
        _run.append((stages, results))
    return _run[0]


@pytest.fixture(scope="module")
def censuses():
    oracle.build(ref=False)
    O = oracle.Oracle()
    return {name: (W.rules_census(O, W.get(name)), R.census(O, W.get(name))) for name in W.SETS}


def route(stages, name):
    lines = stages.get(name, [])
    assert len(lines) == 1, (name, stages)
    m = LEAN.search(lines[0])
    assert m, lines
    rec, layout, touched, lean, left, huge, free = (int(x) if x.isdigit() else x for x in m.groups())
    return {"touched": touched, "lean": lean, "left": left, "huge": huge, "free": free}


@pytest.mark.parametrize("mode", ["", "sat-"])
@pytest.mark.parametrize("name", W.SETS)
def test_route_is_the_census(censuses, name, mode):
    stages, results = run()
    states, clean_census = censuses[name]
    r = route(stages, mode + name)
    lean = sum(s["lean"] for s in states.values())
    free = sum(s["clean"] for s in states.values())
    print(mode + name, r, states)
    assert (clean_census["partitions"], clean_census["LEAN"], clean_census["CLEAN"], clean_census["AMBIG"]) == (len(states), lean, free, 0)  # both censuses
    assert r == {"touched": len(states), "lean": lean, "left": len(states) - lean, "huge": 0, "free": free}, (r, states)
    assert results[mode + name] == results[name]  # (no count near 255: the same entries, counts and digest, each equal to the oracle's: the worker)
