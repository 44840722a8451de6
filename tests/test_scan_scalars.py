"""GPU: what k_scan2 does around its step loop (DESIGN.md section 4 finding 23): the arguments come as one struct, every flush of the emit
queue reads what the record builders need from the kernel-argument segment again, the loop's trip count is a scalar, the flush is a
branch marked rare.  None of it may change a record, so everything here goes through the public counting path at k63 m21 b14 and is
compared with the oracle's index of the same reads (tests/scan_scalars_worker.py: entries, buckets, sum of counts, enumeration,
digest; the queries with the oracle's answers).  The shapes are those at which that code takes another path:

  * mixed: one wave with the lengths k - 1, k, k + 1, k + 30 .. k + 33 and 150 side by side (dead lanes beside live ones, the 32-step
    buffer reload), one whose trip count comes from a single lane, one without any k-mer (straight to the final flush);
  * incomplete-blocks: a read count that is no multiple of 64 nor of 1024;
  * dense: 400-nt reads with errors, a dozen super-k-mers per lane and more: the queue is flushed inside the step loop several times
    and once more at the end.  That a flush inside the loop happened is asserted from the library's record counter, below;
  * queries: the same kinds of reads through the query scan (MODE 1) and the per-position scan (MODE 3);
  * generic: k = 61, which takes the body with run-time k and m.

The worker runs twice: with the emit queue at 320 entries per wave, the library's default at this geometry (set explicitly, so that the
bound asserted here is this file's own), and at 128, the smallest the library takes, where every shape but the first flushes in the loop.

(The exact fold behind the guard band's branch is built with -DCLS_FORCE_GUARD; the suite's build helper, brisk_amd.build_library, takes
no flags, so no test here runs under it.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scan_scalars_worker.py")
QCAPS = (320, 128)
INSERTS = ("mixed", "incomplete-blocks", "dense", "generic")
_runs = {}


def run(qcap):
    if qcap not in _runs:
        env = {k: v for k, v in os.environ.items() if not k.startswith("BRISK_") or k == "BRISK_HIP_LIB"}
        env["BRISK_SCAN_QCAP"] = str(qcap)
        p = subprocess.run([sys.executable, WORKER], env=env, capture_output=True, text=True, timeout=600)
        results = {}
        for line in p.stdout.splitlines():
            k, _, v = line.partition(" ")
            if v:
                results[k] = json.loads(v)
        _runs[qcap] = (p, results)
    return _runs[qcap]


@pytest.mark.parametrize("qcap", QCAPS)
def test_every_shape_is_the_oracles_index(qcap):
    p, results = run(qcap)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (qcap, p.stdout[-3000:], p.stderr[-6000:])
    assert set(results) == set(INSERTS) | {"queries"}
    print(qcap, results)
    assert results["mixed"]["live"] < results["mixed"]["reads"]          # lanes without a k-mer
    assert results["queries"]["found"] > 0 and results["queries"]["found"] < results["queries"]["slots"]


def flushes_in_the_loop(r, qcap):
    """A wave flushes inside the step loop once its queue holds more than qcap - 64 entries at the end of a step; every live read queues
    at most one more super-k-mer after the loop.  With no flush inside the loop the reads' records are therefore at most
    waves * (qcap - 64) + live.  (Eight waves more than the reads fill: were the batch scanned in several launches, each could add a
    partly filled one.)  Returns how many times over that bound the record counter is."""
    waves = (r["reads"] + 63) // 64 + 8
    return (r["records"] - r["live"]) / (waves * (qcap - 64))


@pytest.mark.parametrize("qcap", QCAPS)
def test_the_dense_reads_flush_inside_the_step_loop(qcap):
    p, results = run(qcap)
    assert "dense" in results, (p.stdout[-3000:], p.stderr[-6000:])
    over = flushes_in_the_loop(results["dense"], qcap)
    print(qcap, results["dense"], "records in the loop per wave / flush threshold: %.2f" % over)
    assert over > 2  # not one flush somewhere: the average wave flushes at least twice


def test_the_short_queue_flushes_in_every_larger_shape():
    p, results = run(128)
    for name in ("incomplete-blocks", "generic"):
        assert name in results, (p.stdout[-3000:], p.stderr[-6000:])
        assert flushes_in_the_loop(results[name], 128) > 1, (name, results[name])


def test_the_queue_length_changes_no_index():
    a, b = run(QCAPS[0])[1], run(QCAPS[1])[1]
    for name in INSERTS:
        assert a[name]["digest"] == b[name]["digest"] and a[name]["records"] == b[name]["records"], name
    assert a["queries"] == b["queries"]
