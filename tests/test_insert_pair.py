"""GPU: two small partitions per wave in k_insert_first (DESIGN.md section 4 finding 22).

The cases (tests/insert_pair_reads.py) are crafted neighbouring partitions at k63 m21 b14, each case into a fresh index: the record
limit (32 + 32 pair, 32 + 33 do not), the instance limit (96 + 96, 1 + 191, 128 + 64 pair; 96 + 97 does not: A alone, B heads the next
pair), the same with contained and repeated records, cousin partitions that hold the same strings, mixed paths (a partner for the
table path, one of more than 64 records, an A of more than 192 instances), batch edges (3, 65 and 66 partitions, a single one), three
of them again into a saturating index, and two medium jobs of 20 k reads at about 12 records per partition.  The worker (one child
process per environment) compares every index with the oracle's: full enumeration, nb_kmers, nb_buckets, digest.  This file asserts

  * the route: the library's count of partitions taken in pairs (the BRISK_DEBUG_INSERT line) is what the CPU restatement of the rule
    (tests/insert_pair_rules.py) makes of the oracle's records -- for the crafted cases computed before anything runs on the device,
    for the medium jobs over the touched list in the order the device walked it (the order of its blocks of 8192 partitions is the
    device's; inside a block it is ascending);
  * with BRISK_INSERT_PAIR=0: no pairs, the same digests, the same entries in the directory for every partition, and the same
    capacity for every partition k_insert_first takes (what it leaves over gets a capacity that depends on the order its records
    arrive in, with either route: see the test).  The slices' offsets and the garbage statistic may differ and are not compared."""
import json
import os
import re
import subprocess
import sys

import pytest

import oracle
import insert_pair_reads as PR
import insert_pair_rules as RU
import insert_pair_worker as W

pytestmark = pytest.mark.gpu

PAIRS = re.compile(r"k_insert_first: (\d+) of (\d+) partitions taken in pairs, (\d+) table-free, (\d+) left over")
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "insert_pair_worker.py")
STAGES = tuple(PR.CASES) + tuple("sat-" + n for n in PR.SAT_CASES) + W.MEDIUM
_runs = {}


@pytest.fixture(scope="module")
def predicted():
    """{case: (outcome per partition, records per partition)} of the crafted cases, from the oracle's records alone"""
    oracle.build(ref=False)
    O = oracle.Oracle()
    out = {}
    for name in PR.CASES:
        parts = PR.partitions_of(O, PR.pack(PR.case(name)))
        out[name] = (RU.walk(RU.ascending(parts), parts), parts)
    return out


def run(**env_add):
    key = tuple(sorted(env_add.items()))
    if key in _runs:
        return _runs[key]
    env = {k: v for k, v in os.environ.items() if not k.startswith("BRISK_") or k == "BRISK_HIP_LIB"}
    env.update(BRISK_DEBUG_INSERT="1", **env_add)
    p = subprocess.run([sys.executable, WORKER], env=env, capture_output=True, text=True, timeout=600)
    lines, name = {}, "start"
    for line in p.stderr.splitlines():
        if line.startswith("[lean] stage "):
            name = line.split()[-1]
        elif PAIRS.search(line):
            lines.setdefault(name, []).append(tuple(int(x) for x in PAIRS.search(line).groups()))
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (env_add, p.stdout[-3000:], p.stderr[-6000:])
    results = {}
    for line in p.stdout.splitlines():
        k, _, v = line.partition(" ")
        if v:
            results[k] = json.loads(v)
    _runs[key] = (lines, results)
    return _runs[key]


def route(lines, name):
    got = lines.get(name, [])
    assert len(got) == 1, (name, lines)
    return dict(zip(("pairs", "touched", "free", "left"), got[0]))


@pytest.mark.parametrize("name", tuple(PR.CASES) + tuple("sat-" + n for n in PR.SAT_CASES))
def test_crafted_neighbours_pair_as_the_rule_says(predicted, name):
    outcome, parts = predicted[name[4:] if name.startswith("sat-") else name]  # (computed before the worker is started)
    lines, results = run()
    r, t = route(lines, name), RU.tally(outcome)
    print(name, r, t)
    assert results[name]["touched"] == RU.ascending(parts)
    assert r["touched"] == len(parts) and r["pairs"] == t["pair"] and r["left"] == t["left"], (r, t)
    assert r["free"] == sum(1 for o in outcome.values() if o[0] != "left" and o[2]), (r, outcome)


_medium = {}


def medium_parts(name):
    """{partition: records} of a medium job, from the oracle alone (once per process)"""
    if name not in _medium:
        oracle.build(ref=False)
        O = oracle.Oracle()
        _medium[name] = PR.partitions_of(O, W.medium(O, name))
    return _medium[name]


@pytest.mark.parametrize("name", W.MEDIUM)
def test_medium_jobs_pair_as_the_rule_says(name):
    lines, results = run()
    parts = medium_parts(name)
    order = results[name]["touched"]
    assert sorted(order) == sorted(parts)
    for a, b in zip(order, order[1:]):  # ascending inside a block of the touched list
        assert a < b or a // RU.TOUCHED_BLOCK != b // RU.TOUCHED_BLOCK
    outcome = RU.walk(order, parts)
    r, t = route(lines, name), RU.tally(outcome)
    print(name, r, t, "records per partition %.2f" % (sum(len(v) for v in parts.values()) / len(parts)))
    assert r["touched"] == len(parts) and r["pairs"] == t["pair"] and r["left"] == t["left"], (r, t)
    assert t["pair"] > 0


def grow_cap(n):
    return n + (n >> 2) + 8  # (brisk_partition.hip)


@pytest.mark.parametrize("name", STAGES)
def test_same_index_and_directory_with_the_route_switched_off(predicted, name):
    """(entries, capacity) of every partition k_insert_first takes are equal with the route on and off, and are (n, grow_cap(n)): a
    fresh partition's one slice.  A partition it leaves over -- more than 64 records or 192 instances -- is filled by
    k_insert_fast_listed chunk by chunk; its slice grows with the new entries each chunk of 64 records brings, and the records
    arrive in the order the scatter's atomics land, so its capacity differs between two runs of the SAME route (the parent's
    too: two inserts of the medium synthetic job with the single-partition body, -DINSERT_PAIR=0, gave 365 of its 371 left-over
    partitions another capacity, none of the 7,488 others, and every partition the same entries).  For those the entries are compared, and the capacity only has to hold them."""
    lines, results = run()
    off_lines, off = run(BRISK_INSERT_PAIR="0")
    assert route(off_lines, name)["pairs"] == 0
    a, b = route(lines, name), route(off_lines, name)
    assert (a["touched"], a["free"], a["left"]) == (b["touched"], b["free"], b["left"]), (a, b)
    assert results[name]["digest"] == off[name]["digest"]  # (each equal to the oracle's: the worker)
    on_dir = dict(zip(results[name]["touched"], zip(results[name]["cnt"], results[name]["cap"])))
    off_dir = dict(zip(off[name]["touched"], zip(off[name]["cnt"], off[name]["cap"])))
    assert sorted(on_dir) == sorted(off_dir)
    base = name[4:] if name.startswith("sat-") else name
    parts = medium_parts(name) if name in W.MEDIUM else predicted[base][1]
    left = {p for p, recs in parts.items() if len(recs) > RU.MAX_REC or RU.single(recs)[2] > RU.MAXI}
    assert len(left) == a["left"]
    for p in on_dir:
        if p in left:
            assert on_dir[p][0] == off_dir[p][0] and on_dir[p][0] <= min(on_dir[p][1], off_dir[p][1]), (p, on_dir[p], off_dir[p])
        else:
            assert on_dir[p] == off_dir[p] == (on_dir[p][0], grow_cap(on_dir[p][0])), (p, on_dir[p], off_dir[p])
