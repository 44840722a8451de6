"""GPU: the HIP paths against the CPU oracle at working density, on error-bearing reads.

The other oracle comparisons stop at a few thousand reads: with 2^22 .. 2^24 partitions nearly every partition then holds no
record or one.  Here one batch is large enough for the scan to bin its records by itself (no BRISK_BINS, BRISK_HUGE_AT,
BRISK_INSERT_GENERIC or other forcing switch: the parent removes every BRISK_* variable but BRISK_TRACE), and the reads carry
substitutions, N cuts, pieces shorter than k, a repeat family, tandem reads and lower case (tests/density_reads.py).  Each
case is one child process (tests/density_parity_worker.py) started with BRISK_TRACE=1; the parent asserts from the library's
`[brisk_hip] path:` lines that the batch took the path the case exists for.

case  geometry, options                 reads     must be seen in the trace of the one-call insert
A     k31 m15 b14, part_bits=22         600 k     binned scan, > 0 records beyond their bins, insert on the binned layout
B     k63 m21 b14, part_bits=20         400 k     binned scan; routing shift 8, which no compile-time insert body has
C     k31 m11 b11, defaults             500 k     records to staging then k_scatter; k_insert_big; > 0 partitions to k_insert_huge
D     k63 m21 b14, 2^24 partitions      5.5 M     binned scan, insert on the binned layout (k_insert_fast<3,49,4>'s geometry)

A-C run at a substitution rate of 1 % and error-free (C at 0.1 % as well: see its test), D at 0.1 %.

Read counts.  scan_binned takes a batch when records_estimate >= 2 * partitions (18.7 records per read at k31 m15, 7.5 at k63
m21 with this length mix).  One more condition stands before it: with default options a batch of fewer than 10 records per
partition is a deferred insert (defer_batch), scanned into the pending buffer and flushed through the classic layout -- the
binned insert of case D would need 24 M reads in one call.  So the index whose trace is asserted is created with the public
option immediate_inserts (brisk_hip_options), which is what a caller who inserts one batch per call sets; the partitions, bin
sizes and kernels are the defaults'.  The default, deferring options are exercised by the third build below.

Per case, against the oracle over 16 threads (bit-exact; all of it is integer work):
* the index built three ways -- one insert_packed call from device memory, one insert_flat call (host upload), and with default
  options three uneven batches in another order: checksum() == the oracle's digest, nb_kmers and nb_buckets equal.  For D the
  oracle runs twice with a bucket filter (two disjoint sixteenths of the bucket space, picked by the seed; an unfiltered table
  of 135 M entries would take 8 GB): enumerate() cut to each range by bo_bucket_ids must have the oracle's digest and bucket
  count, and the unfiltered total is pinned by sum of counts == sum(max(0, len - k + 1)).
* get_reads / get_packed per-read sums over >= 200 k queries (A: 520 k, enough for the binned query scan; inserted reads, reads with fresh substitutions, reads of another
  genome, poly-A runs that meet the minimizer == 0 stop) == the oracle's (A-C);
* get_kmers_packed == get_kmers on that query set, and get_kmers slot by slot == expected_all of tests/test_kmer_query.py on
  2000 of its reads (D: on the slots the filtered oracle knows, and every k-mer of an inserted read present);
* after a second insert of the same batch: entries unchanged, digest == the oracle's after its own second insert.

A mismatch prints the differing entries as `KMER idx count` lines and the trace.

Cost, measured: on a 16-thread CPU-only host the oracle's insert takes 7.1 s (A), 3.8 s (B), 3.3 s (C) and 25 s per bucket
range (D), its query of 200 k reads 1.3-1.6 s, peak RSS 3.4 GB (A), 3.0 GB (B), 2.0 GB (C), 3.9 GB (D, filtered; the read
generator takes 37 s there).  On the MI355X host the whole module (8 children) takes 97 s of wall time, D 31 s of it; the
rest of the `-m gpu` suite takes 199 s.  Nothing of D had to be cut."""
import os
import re
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "density_parity_worker.py")


def run_case(case, e, timeout):
    env = {k: v for k, v in os.environ.items() if not k.startswith("BRISK_") or k == "BRISK_HIP_LIB"}
    env["BRISK_TRACE"] = "1"
    t0 = time.time()
    p = subprocess.run([sys.executable, WORKER, case, str(e)], env=env, capture_output=True, text=True, timeout=timeout)
    print(f"case {case} e={e}: {time.time() - t0:.0f} s")
    print(p.stdout)
    stages, name = {}, "start"
    for line in p.stderr.splitlines():
        if line.startswith("[density] stage "):
            name = line.split()[-1]
        elif line.startswith("[brisk_hip] path:"):
            stages.setdefault(name, []).append(line)
    trace = "\n".join(f"{s}: {l}" for s, ls in stages.items() for l in ls)
    print(trace)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (case, e, p.stdout[-6000:], p.stderr[-6000:])
    results = {}
    for line in p.stdout.splitlines():
        key, _, val = line.partition(" ")
        results[key] = val
    return stages, results, trace


def _one(lines, pattern, trace):
    hits = [m for m in (re.search(pattern, l) for l in lines) if m]
    assert hits, (pattern, trace)
    return hits


def assert_binned(stages, trace, n_reads, n_parts, beyond_bins):
    lines = stages.get("packed", [])
    m = _one(lines, r"binned scan of (\d+) reads: (\d+) records, bins of (\d+), (\d+) records beyond their bins", trace)[0]
    assert int(m.group(1)) == n_reads, trace  # the whole batch in one scan
    # bins sized by the batch: (2 * estimate / partitions + 8) rounded up to 4, the estimate within [1, 2] x the records
    assert 12 <= int(m.group(3)) <= 4 * int(m.group(2)) // n_parts + 12, trace
    if beyond_bins:
        assert int(m.group(4)) > 0, trace
    _one(lines, r"insert of \d+ records \(binned layout", trace)
    _one(lines, r"direct insert of %d reads, records binned by the scan" % n_reads, trace)
    assert not any("k_scatter" in l or "deferred" in l for l in lines), trace
    return m


def _n_reads(results):
    import json
    return json.loads(results["reads"])["n"]


@pytest.mark.parametrize("e", [0.01, 0.0])
def test_case_a_k31_m15_binned_with_overflow(e):
    stages, results, trace = run_case("A", e, 900)
    assert_binned(stages, trace, _n_reads(results), 1 << 22, beyond_bins=True)
    # the second insert of the batch meets a full index on the same path
    _one(stages.get("second", []), r"insert of \d+ records \(binned layout", trace)
    if e > 0:  # 490 k queries without the poly-A reads are dense enough for the binned query scan (k_query_fast over bins)
        _one(stages.get("get_packed-dense", []), r"binned scan of \d+ reads", trace)


@pytest.mark.parametrize("e", [0.01, 0.0])
def test_case_b_k63_m21_runtime_geometry_on_natural_bins(e):
    import json
    stages, results, trace = run_case("B", e, 900)
    assert_binned(stages, trace, _n_reads(results), 1 << 20, beyond_bins=False)
    lay = json.loads(results["layout"])
    # routing id bits kept in the entry key: 2b + ext_bits - part_bits = 8; the compile-time bodies for (nw 3, k - b 49) exist
    # for 1..4 only (brisk_capi.hip, LAUNCH_INSERT_FAST), so this insert ran the run-time-geometry body
    # (record_words counts the header word: 3 payload words)
    assert (lay["record_words"], lay["k"] - lay["b"], 2 * lay["b"] + lay["ext_bits"] - lay["part_bits"]) == (4, 49, 8), lay


@pytest.mark.parametrize("e", [0.01, 0.001, 0.0])
def test_case_c_k31_m11_big_and_huge_partitions(e):
    """k_insert_big is chosen at more than 64 records per touched partition.  At e = 1 % no batch reaches that with this
    geometry: a read of 150 bp makes about 18 records and carries 1.5 errors, each of which touches about 0.46 partitions no
    other read touches -- at most 18 / 0.69 = 26 records per touched partition however many reads there are (measured: 22).
    So the 1 % run asserts the staging path and k_insert_huge, and k_insert_big is asserted at 0.1 % and error-free."""
    import json
    stages, results, trace = run_case("C", e, 900)
    lines = stages.get("packed", [])
    _one(lines, r"direct insert of %d reads, records to staging, then k_scatter" % _n_reads(results), trace)
    m = _one(lines, r"insert of (\d+) records \(classic layout.* into (\d+) partitions: (k_insert\w*).*, (\d+) partitions to k_insert_huge", trace)[0]
    if e <= 0.001:
        assert m.group(3) == "k_insert_big" and int(m.group(1)) > 64 * int(m.group(2)), trace
    assert int(m.group(4)) > 0, trace
    # by the oracle's enumerator alone, a part of the batch already puts more instances than the default threshold (16384)
    # into one partition
    assert json.loads(results["hottest_group"]) > 16384, results["hottest_group"]
    assert json.loads(results["layout"])["cls_bits"] == 1


def test_case_d_k63_m21_all_default_partitions():
    import json
    stages, results, trace = run_case("D", 0.001, 1500)
    assert_binned(stages, trace, _n_reads(results), 1 << 24, beyond_bins=False)
    lay = json.loads(results["layout"])
    assert (lay["part_bits"], lay["record_words"], lay["k"] - lay["b"], 2 * lay["b"] + lay["ext_bits"] - lay["part_bits"]) == (24, 4, 49, 4), lay
    _one(stages.get("second", []), r"insert of \d+ records \(binned layout", trace)
