"""GPU: k_insert_first, the first fill of empty partitions (DESIGN.md section 4 finding 16).

The first insert into a fresh k63 index runs k_insert_first over all touched partitions, then k_insert_fast over the partitions
it left over (not empty, more than 64 records, or more than 64 * NI_LEAN instances after the containment fold), then
k_insert_huge.  Whatever the route, the index must be the oracle's: every case compares the full enumeration (k-mer,
minimizer_idx, count), nb_kmers, nb_buckets and the digest in the worker (tests/insert_lean_worker.py: one child process per
environment, since the library reads its switches once), and the parent asserts from the library's `[brisk_hip] path:` lines
that each insert took the route the case exists for.

Shapes: k63 m21 b14 at the default 2^24 partitions (the compile-time bodies exist for routing shifts 1..4 only, so fewer
partitions would take the run-time body).  Density therefore comes from the genome, not from part_bits: 8,000 reads of a 24 kb
genome.  The worker counts, with the oracle on the CPU, the partitions that hold more than 128 distinct k-mers (they cannot
fit 64 * NI_LEAN instance slots however their records fold) and those of more than 64 records: k_insert_first must leave at
least that many over, and at most half of all partitions -- a lean body that refused everything would pass nothing here."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "insert_lean_worker.py")
LEAN = re.compile(r"insert of (\d+) records \((\w+) layout.* into (\d+) partitions: k_insert_first \(fresh index\): (\d+) partitions lean, (\d+) left over to k_insert, "
                  r"(\d+) partitions to k_insert_huge")
GENERAL = re.compile(r"insert of (\d+) records \((\w+) layout.* into (\d+) partitions: k_insert, (\d+) partitions to k_insert_huge")
# What the build keeps resident (brisk_insert.hip): the six-wave body, 24 waves per CU.  (Had the 80-register body needed
# scratch, the 96-register one would have been kept instead and 20 expected here.)  The library reports the smaller of the
# occupancy query's answer and the 24 the kernel is built for: fewer than 24 means its registers or LDS no longer allow six.
WAVES_PER_CU = 24

_runs = {}


def run(scenario, **env_add):
    """one child per (scenario, environment), shared by the tests that read it"""
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
        elif line.startswith("[brisk_hip]"):
            stages.setdefault(name, []).append(line)
    trace = "\n".join(f"{s}: {l}" for s, ls in stages.items() for l in ls)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (scenario, env_add, p.stdout[-3000:], p.stderr[-6000:])
    results = {}
    for line in p.stdout.splitlines():
        k, _, v = line.partition(" ")
        if v:
            results[k] = json.loads(v)
    _runs[key] = (stages, results, trace)
    return _runs[key]


def inserts(stages, name, trace):
    lines = [l for l in stages.get(name, []) if "path: insert of" in l]
    assert lines, (name, trace)
    return lines


def lean_line(stages, name, trace):
    lines = inserts(stages, name, trace)
    assert len(lines) == 1, (name, trace)
    m = LEAN.search(lines[0])
    assert m, (name, trace)
    rec, layout, touched, lean, left, huge = m.groups()
    assert int(lean) + int(left) + int(huge) == int(touched), trace
    return {"layout": layout, "touched": int(touched), "lean": int(lean), "left": int(left), "huge": int(huge)}


def general_lines(stages, name, trace):
    lines = inserts(stages, name, trace)
    for l in lines:
        assert GENERAL.search(l) and "k_insert_first" not in l, (name, trace)
    return lines


def test_first_batch_goes_lean_and_leaves_the_large_partitions_over():
    stages, results, trace = run("main", BRISK_DEBUG_INSERT="1")
    r = lean_line(stages, "first", trace)
    ra = results["reads_a"]
    assert r["layout"] == "classic" and r["touched"] == ra["partitions"] and r["huge"] == 0, (r, ra, trace)
    # the reads were chosen so that a few partitions cannot go lean: checked with the oracle's per-partition numbers
    assert ra["over"] >= 5 and ra["many_records"] >= 5 and ra["records_per_partition"] > 6, ra
    assert r["lean"] > 0 and max(ra["over"], ra["many_records"]) <= r["left"] <= r["touched"] // 2, (r, ra)


def test_same_reads_with_the_lean_route_switched_off():
    stages, results, trace = run("main", BRISK_DEBUG_INSERT="1")
    off_stages, off, off_trace = run("one-batch", BRISK_INSERT_LEAN="0")
    general_lines(off_stages, "first", off_trace)
    assert off["first"] == results["first"]  # entries, sum of counts, digest


def test_second_batch_is_general_and_clear_restores_the_route():
    stages, results, trace = run("main", BRISK_DEBUG_INSERT="1")
    general_lines(stages, "second", trace)
    again, first = lean_line(stages, "again", trace), lean_line(stages, "first", trace)
    # (the records of a partition arrive in another order, so a partition at the edge of 64 * NI_LEAN instances may fold otherwise)
    assert again["touched"] == first["touched"] and again["lean"] > 0 and again["left"] <= again["touched"] // 2, (again, first)


def test_flag_is_conservative_after_load_and_merge():
    stages, results, trace = run("main", BRISK_DEBUG_INSERT="1")
    general_lines(stages, "after-load", trace)
    general_lines(stages, "merge", trace)
    general_lines(stages, "after-merge", trace)


def test_partition_of_more_than_64_records_is_left_over():
    stages, results, trace = run("main", BRISK_DEBUG_INSERT="1")
    r = lean_line(stages, "many-records", trace)
    first = lean_line(stages, "first", trace)
    more = results["sub_reads"]["many_records"] - results["reads_a"]["many_records"]
    assert more > 0 and r["lean"] > 0 and results["sub_reads"]["many_records"] <= r["left"] <= r["touched"] // 2, (r, first, results)


def test_partitions_of_k_insert_huge_are_skipped():
    stages, results, trace = run("one-batch", BRISK_HUGE_AT="800")
    r = lean_line(stages, "first", trace)
    assert r["huge"] > 0 and r["lean"] > 0, r


def test_binned_layout_with_overflow_records():
    """(a read set of its own: the overflow area of a forced binned scan is small, and reads_a's hottest partitions exceed it)"""
    stages, results, trace = run("one-batch-c", BRISK_BINS="8")
    r = lean_line(stages, "first", trace)
    assert r["layout"] == "binned" and r["lean"] > 0, r
    m = [re.search(r"binned scan of \d+ reads: \d+ records, bins of 8, (\d+) records beyond their bins", l) for l in stages.get("first", [])]
    assert any(x and int(x.group(1)) > 1000 for x in m), trace
    assert lean_line(run("one-batch-c")[0], "first", trace)["layout"] == "classic"
    assert results["first"] == run("one-batch-c")[1]["first"]  # (the classic layout's)


def test_saturating_index():
    stages, results, trace = run("main", BRISK_DEBUG_INSERT="1")
    assert lean_line(stages, "sat", trace)["lean"] > 0  # (the counts -- 255 for every k-mer of the read seen 300 times -- are checked in the worker)


def test_deferred_inserts_complete_lean():
    stages, results, trace = run("main", BRISK_DEBUG_INSERT="1")
    assert not [l for l in stages.get("deferred-calls", []) if "path: insert of" in l], trace
    assert len([l for l in stages.get("deferred-calls", []) if "deferred scan" in l]) == 3, trace
    assert any("flush of" in l for l in stages.get("deferred-complete", [])), trace
    r = lean_line(stages, "deferred-complete", trace)
    assert r["touched"] == lean_line(stages, "first", trace)["touched"] and r["lean"] > 0 and r["left"] <= r["touched"] // 2, r


def test_resources_of_the_lean_kernel():
    stages, results, trace = run("main", BRISK_DEBUG_INSERT="1")
    m = [re.search(r"k_insert_first: (\d+) waves per CU, (\d+) registers, (\d+) B of LDS, (\d+) B of scratch", l) for l in stages.get("first", [])]
    m = [x for x in m if x]
    assert m, trace
    waves, regs, lds, scratch = (int(x) for x in m[0].groups())
    assert (waves, scratch) == (WAVES_PER_CU, 0) and regs <= 80 and lds <= 13 * 512, m[0].group(0)
