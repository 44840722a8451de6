"""Worker of tests/test_density_parity.py: one dense, error-bearing batch through the HIP paths, against the threaded oracle.

usage: density_parity_worker.py CASE ERROR_RATE      (CASE in A B C D; see CASES and the test module's docstring)

The parent starts it with BRISK_TRACE=1 and reads the library's `[brisk_hip] path:` lines from stderr; this process writes a
`[density] stage NAME` line to stderr before every stage so that the parent knows which call a path line belongs to.  stdout
carries `key value` result lines and ends with `ok`; a mismatch prints the differing entries (density_reads.entry_diff) and
exits 1."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import brisk_amd
import oracle
from density_reads import as_strings, concat_reads, dense_reads, entry_diff, poly_a_reads, substitute, take_reads

THREADS = 16  # the oracle's; not os.cpu_count(): a test host gives a process a share of its cores

# geometry, index options, reads, genome length, generator extras.  Read counts: tests/test_density_parity.py.
# The repeat families of A and B are small on purpose: the binned scan keeps the records beyond the bins in 4096 regions of
# (estimate / 8 + 65536) / 4096 slots (383 for A, 107 for B), a partition's overflow goes to one region, and a region that
# runs full sends the whole batch to the classic path.  8 (4) copies at coverage 15 put about 100 (45) records into the
# partitions of the element's minimizers, against a mean of 6 (3): an order of magnitude, and two of them still fit a region.
CASES = {
    "A": dict(kmb=(31, 15, 14), opts=dict(part_bits=22), n=600_000, genome=6_000_000, genome_error_free=24_000_000, gen=dict(repeat_len=1000, repeat_copies=8, n_special=60)),
    "B": dict(kmb=(63, 21, 14), opts=dict(part_bits=20), n=400_000, genome=4_000_000, gen=dict(repeat_len=1000, repeat_copies=4, n_special=60)),
    "C": dict(kmb=(31, 11, 11), opts=dict(), n=500_000, genome=500_000, gen=dict(repeat_len=1000, repeat_copies=100)),
    "D": dict(kmb=(63, 21, 14), opts=dict(), n=5_500_000, genome=80_000_000, gen=dict(n_special=0)),
}
N_QUERY = {"A": 520_000, "B": 200_000, "C": 200_000, "D": 200_000}
N_SLOT_SAMPLE = 2000


def stage(name):
    sys.stdout.flush()
    sys.stderr.write(f"[density] stage {name}\n")
    sys.stderr.flush()


def say(key, value):
    print(key, json.dumps(value), flush=True)


def fail(what, detail=""):
    print("MISMATCH", what, flush=True)
    if detail:
        print(detail, flush=True)
    sys.exit(1)


def to_device(ix, flat, offs):
    d_bases = torch.from_numpy(flat).cuda()
    d_packed = torch.zeros((len(flat) + 15) // 16 + 4, dtype=torch.int32, device="cuda")
    d_starts = torch.from_numpy(offs.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    ix.pack_ascii(d_bases.data_ptr(), len(flat), d_packed.data_ptr())
    ix.sync()
    del d_bases
    return d_packed, d_starts


def get_reads_flat(ix, flat, offs):
    out = np.zeros(len(offs) - 1, np.uint64)
    ix._chk(ix.L.brisk_hip_get_reads(ix.h, flat, offs, len(offs) - 1, out))
    return out


def get_kmers_flat(ix, flat, offs):
    total = int(brisk_amd.kmer_slots(offs, ix.k)[-1])
    out = np.zeros(max(total, 1), np.uint16)
    ix._chk(ix.L.brisk_hip_get_kmers(ix.h, flat, offs, len(offs) - 1, out, total))
    return out[:total]


def hottest_group(O, flat, offs, k, m, cls_bits, cls_width, which):
    """A lower bound, from the oracle's enumerator alone, on the k-mer instances of the fullest partition: the instances of
    the reads `which` that share a minimizer and a minimizer_idx class -- the library routes by the hashed minimizer and that
    class, so they all lie in one partition."""
    assert k <= 32
    keys = []
    for s in as_strings(*take_reads(flat, offs, which)):
        if len(s) < k:
            continue
        _, _, lo, _, idx, _ = O.enumerate(s, k, m)
        mm = (lo >> (2 * idx.astype(np.uint64))) & np.uint64((1 << (2 * m)) - 1)  # the m-mer at minimizer_idx (Kmers.cpp:191-200)
        cls = (idx // cls_width).astype(np.uint64) if cls_bits else np.zeros(len(idx), np.uint64)
        keys.append(mm * np.uint64(64) + cls)
    _, counts = np.unique(np.concatenate(keys), return_counts=True)
    return int(counts.max())


def main():
    case, e = sys.argv[1], float(sys.argv[2])
    cfg = CASES[case]
    k, m, b = cfg["kmb"]
    seed = 1000 * (ord(case) - 64) + int(round(e * 10000))
    t_all = time.time()
    oracle.build(ref=False)
    O = oracle.Oracle()
    t0 = time.time()
    # (error-free reads at coverage 15 put 15 records into every partition they touch: more lie beyond bins of 16 than the
    # overflow area holds, and the batch takes the classic path; A's error-free run samples a genome four times as long)
    genome_len = cfg.get("genome_error_free", cfg["genome"]) if e == 0 else cfg["genome"]
    flat, offs = dense_reads(cfg["n"], k, genome_len, seed, e=e, **cfg["gen"])
    n = len(offs) - 1
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    instances = int(np.maximum(lens - k + 1, 0).sum())
    say("reads", dict(n=n, bases=len(flat), shorter_than_k=int((lens < k).sum()), instances=instances, gen_s=round(time.time() - t0, 1)))

    # ---- the oracle: whole for A-C, two bucket ranges of 1/16 of the bucket space for D
    n_buckets = 1 << (2 * b)
    ranges = [None]
    if case == "D":
        rng = np.random.default_rng(seed)
        i, j = rng.choice(16, 2, replace=False)
        ranges = [(int(i) * n_buckets // 16, (int(i) + 1) * n_buckets // 16), (int(j) * n_buckets // 16, (int(j) + 1) * n_buckets // 16)]
    t0 = time.time()
    oh = []
    for r in ranges:
        h = O.index_new(k, m, b)
        if r:
            O.index_set_bucket_range(h, *r)
        O.index_insert_reads(h, flat, offs, threads=THREADS)
        oh.append(h)
    want = [O.index_digest(h) for h in oh]
    want_stats = [O.index_stats(h) for h in oh]
    say("oracle", dict(insert_s=round(time.time() - t0, 1), ranges=ranges, digest=want, stats=want_stats))

    def check_index(ix, what):
        """checksum / stats against the oracle (D: the enumeration cut to the oracle's bucket ranges, and the unfiltered total)"""
        cs, st = ix.checksum(), ix.stats()
        say(what, dict(checksum=cs, nb_kmers=st["nb_kmers"], nb_buckets=st["nb_buckets"]))
        if ranges[0] is None:
            if cs != want[0] or (st["nb_kmers"], st["nb_buckets"]) != want_stats[0]:
                fail(f"{what}: checksum {cs} stats {(st['nb_kmers'], st['nb_buckets'])}, oracle {want[0]} {want_stats[0]}",
                     entry_diff(ix.enumerate(), O.index_dump(oh[0]), k))
            return
        if cs[1] != expected_sum[0]:
            fail(f"{what}: sum of counts {cs[1]}, k-mer instances inserted {expected_sum[0]}")
        if cs[0] != st["nb_kmers"]:
            fail(f"{what}: checksum counts {cs[0]} entries, stats {st['nb_kmers']}")
        all_entries = ix.enumerate(chunk=1 << 24)
        ids = O.bucket_ids(oh[0], all_entries[0], all_entries[1], all_entries[2], threads=THREADS)
        for r, h, w, ws in zip(ranges, oh, want, want_stats):
            inside = (ids >= r[0]) & (ids < r[1])
            cut = tuple(a[inside] for a in all_entries)
            got = O.digest_entries(*cut)
            if got != w or len(np.unique(ids[inside])) != ws[1]:
                fail(f"{what}: bucket range {r}: digest {got} buckets {len(np.unique(ids[inside]))}, oracle {w} {ws}", entry_diff(cut, O.index_dump(h), k))

    expected_sum = [instances]
    opts = cfg["opts"]

    # ---- build 1: device memory, one insert_packed call, inserts immediate (the path the case exists for)
    stage("packed")
    ix = brisk_amd.BriskHip(k, m, b, immediate_inserts=True, **opts)
    say("layout", ix.layout)
    d_packed, d_starts = to_device(ix, flat, offs)
    t0 = time.time()
    ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
    ix.sync()
    say("insert_packed_s", round(time.time() - t0, 2))
    stage("packed-check")
    check_index(ix, "packed")

    if case == "C":  # the fullest partition must lie above the k_insert_huge threshold by the oracle's own count
        stage("hottest")
        sample = np.arange(0, min(n, 150_000))  # (a part of the batch: the bound only gets lower)
        say("hottest_group", hottest_group(O, flat, offs, k, m, ix.layout["cls_bits"], ix.layout["cls_width"], sample))

    # ---- build 2: host memory, one insert_flat call (the upload path), inserts immediate
    stage("host")
    with brisk_amd.BriskHip(k, m, b, immediate_inserts=True, **opts) as ix2:
        ix2.insert_flat(flat, offs)
        stage("host-check")
        check_index(ix2, "host")

    # ---- build 3: default options (small batches are deferred and flushed together), three uneven batches, another order
    stage("batches")
    with brisk_amd.BriskHip(k, m, b, **opts) as ix3:
        c1, c2 = n // 2, n // 2 + n // 7
        for a, z in ((c2, n), (0, c1), (c1, c2)):
            ix3.insert_flat(flat, np.ascontiguousarray(offs[a:z + 1]))
        stage("batches-check")
        check_index(ix3, "batches")

    # ---- queries
    stage("queries")
    rng = np.random.default_rng(seed + 1)
    nq = N_QUERY[case]
    inserted = take_reads(flat, offs, rng.integers(0, n, nq * 2 // 5))
    half = take_reads(flat, offs, rng.integers(0, n, nq * 3 // 10))
    half = (substitute(half[0], 0.02, seed + 2), half[1])  # fresh substitutions: about half of a read's k-mers stay present
    unseen = dense_reads(nq // 4, k, 3_000_000, seed + 3, e=0.0, n_special=0)
    poly = poly_a_reads(nq // 20 + 1000, k, seed + 4)
    qf, qo = concat_reads([inserted, half, unseen, poly])
    say("queries", len(qo) - 1)
    assert len(qo) - 1 >= nq
    q_packed, q_starts = to_device(ix, qf, qo)
    if ranges[0] is None:
        t0 = time.time()
        want_q = O.index_query_reads(oh[0], qf, qo, threads=THREADS)
        say("oracle_query_s", round(time.time() - t0, 1))
        stage("get_reads")
        got = get_reads_flat(ix, qf, qo)
        if not np.array_equal(got, want_q):
            bad = np.nonzero(got != want_q)[0]
            fail(f"get_reads: {len(bad)} reads differ, first {int(bad[0])}: {int(got[bad[0]])} want {int(want_q[bad[0]])}", as_strings(*take_reads(qf, qo, bad[:3]))[0])
        stage("get_packed")
        sums = torch.full((len(qo) - 1,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ix.get_packed(q_packed.data_ptr(), q_starts.data_ptr(), len(qo) - 1, sums.data_ptr())
        got = sums.cpu().numpy().astype(np.uint64)
        if not np.array_equal(got, want_q):
            bad = np.nonzero(got != want_q)[0]
            fail(f"get_packed: {len(bad)} reads differ, first {int(bad[0])}: {int(got[bad[0]])} want {int(want_q[bad[0]])}")
        # the same without the poly-A reads (the last of the set): thousands of them in one partition overflow a region of the
        # binned query scan, which then leaves the whole set to the classic one; without them a dense set stays binned
        stage("get_packed-dense")
        n_dense = len(qo) - len(poly[1])
        sums.fill_(-1)
        torch.cuda.synchronize()
        ix.get_packed(q_packed.data_ptr(), q_starts.data_ptr(), n_dense, sums.data_ptr())
        if not np.array_equal(sums.cpu().numpy().astype(np.uint64)[:n_dense], want_q[:n_dense]):
            fail("get_packed without the poly-A reads differs from the oracle")
        say("query_sums", dict(total=int(want_q.sum()), zero=int((want_q == 0).sum())))
    stage("get_kmers")
    slots = get_kmers_flat(ix, qf, qo)
    d_out = torch.full((max(len(slots), 1),), 0x7777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ix.get_kmers_packed(q_packed.data_ptr(), q_starts.data_ptr(), len(qo) - 1, d_out.data_ptr())
    if not np.array_equal(d_out.cpu().numpy().view(np.uint16)[:len(slots)], slots):
        fail("get_kmers_packed differs from get_kmers")
    say("slots", dict(n=len(slots), found=int(((slots & 0x100) != 0).sum())))
    # slot by slot on a sample (the expectation walks k-mers in Python: tests/test_kmer_query.py)
    stage("get_kmers-sample")
    from test_kmer_query import assert_slots, expected_all
    pick = np.sort(rng.choice(len(qo) - 1, N_SLOT_SAMPLE, replace=False))
    sf, so = take_reads(qf, qo, pick)
    got = get_kmers_flat(ix, sf, so)
    if ranges[0] is None:
        want_s, alts, base = expected_all(O, oh[0], [s.upper() for s in as_strings(sf, so)], k, m)
        assert np.array_equal(base, brisk_amd.kmer_slots(so, k))
        assert_slots(got, want_s, alts, (case, "get_kmers sample"))
    else:
        # a bucket-filtered oracle knows the k-mers of its range only: where it has one, presence and count must agree; and
        # every k-mer of a read that was inserted is present
        for h in oh:
            want_s, alts, base = expected_all(O, h, [s.upper() for s in as_strings(sf, so)], k, m)
            known = want_s != 0
            for s0, e0, _ in alts:  # (a span that is its own reverse complement fits both ways: left to the small-input tests)
                known[s0:e0] = False
            if not np.array_equal(got[known], want_s[known]):
                fail(f"get_kmers sample: {int((got[known] != want_s[known]).sum())} slots of the oracle's bucket range differ")
        n_ins = int((pick < nq * 2 // 5).sum())
        ins_slots = int(brisk_amd.kmer_slots(so, k)[n_ins])
        if not ((got[:ins_slots] & 0x100) != 0).all():
            fail("get_kmers sample: a k-mer of an inserted read is absent")
    say("slot_sample", dict(reads=len(pick), slots=len(got), found=int(((got & 0x100) != 0).sum())))

    # ---- the same batch again: entries unchanged, counts doubled mod 256
    stage("second")
    before = ix.checksum()
    ix.insert_packed(d_packed.data_ptr(), d_starts.data_ptr(), n)
    ix.sync()
    for h in oh:
        O.index_insert_reads(h, flat, offs, threads=THREADS)
    want[:] = [O.index_digest(h) for h in oh]
    if [O.index_stats(h) for h in oh] != want_stats:
        fail("oracle: a second insert of the same batch changed its entries")
    expected_sum[0] = 2 * instances
    stage("second-check")
    check_index(ix, "second")
    if ix.checksum()[0] != before[0]:
        fail(f"second insert: {ix.checksum()[0]} entries, {before[0]} before")
    ix.close()
    say("wall_s", round(time.time() - t_all, 1))
    print("ok", flush=True)


if __name__ == "__main__":
    main()
