"""The device side of tests/test_minimizer_mode.py, run in a child process: every case of full-width minimizers
(brisk_hip_options.minimizer_mode) against the Python restatement of the enumerator (tests/minimizer_reference.py) or a host set --
never against the library itself.

    python tests/minimizer_mode_worker.py OUT.json [case ...]

Runs the named cases (default: all), writes {case: "ok ..." or the failure's traceback} to OUT.json and prints "done <n>"."""
import json
import os
import random
import subprocess
import sys
import tempfile
import traceback
from collections import Counter
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import minimizer_reference as MR  # noqa: E402

EINVAL, EFORMAT = 1, 8
# the smallest geometries at which the new re-scan can go wrong: k33 (the k-mer is truncated in the reference, the (k-1)-mer is not), k34,
# k47 m21, the flagship, k63 m31 (33 windows: one more than a half-wave), k63 m3 b3 (61 windows: the most a wave must hold), k31 m15
# (both modes one function); and one geometry for each unrolled chunk count the full-mode scan is instantiated for that the others
# leave out (m17: four chunks, m27: six)
GEOMETRIES = [(33, 15, 9), (34, 11, 5), (47, 21, 10), (63, 21, 14), (63, 31, 12), (63, 3, 3), (31, 15, 14), (35, 17, 8), (41, 27, 9)]
LONG_AT = {(63, 21, 14), (33, 15, 9)}  # where the chunked sequences join the parity reads
K, M, B_ = 63, 21, 14


def brisk():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


def parity_input(k, long_too):
    """a few hundred reads: random ones of k, k + 1, 2k - 1 and 150 nt from either strand of a 3 kb genome, the periodic and
    homopolymer reads of the tie tests, and (long_too) sequences of more than 8192 k-mers, which are scanned in chunks -- a random
    one (seams that match) and one with a tandem stretch (seams that do not: seeded re-runs)"""
    rng = random.Random(77 + k)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    g = rnd(3000)
    reads = []
    for i in range(160):
        n = (k, k + 1, 2 * k - 1, 150)[i % 4]
        p = rng.randrange(len(g) - n + 1)
        reads.append(MR.revcomp(g[p:p + n]) if rng.random() < 0.5 else g[p:p + n])
    reads += [r for r in MR.parity_reads() if len(r) >= k]
    if long_too:
        reads += [rnd(12_288 + 62), rnd(3000) + "ACGTTGCA" * 1100 + rnd(3000)]
    return reads


def entries(ix):
    lo, hi, idx, cnt = ix.enumerate()
    got = Counter()
    for ident, c in zip(zip(lo.tolist(), hi.tolist(), idx.tolist()), cnt.tolist()):
        assert ident not in got, "one identity, two entries"
        got[ident] = c
    return got


def case_parity(B, k, m, b, full):
    reads = parity_input(k, (k, m, b) in LONG_AT)
    want = {ident: (2 * c) % 256 for ident, c in MR.index_of(reads, k, m, full).items()}  # each read inserted twice; the count byte wraps
    with B.BriskHip(k, m, b, minimizer_mode="full" if full else "reference") as ix:
        ix.insert_reads(reads)
        ix.insert_reads(reads)
        got = entries(ix)
    assert len(got) == len(want), (len(got), len(want))
    assert got == want, [(i, got.get(i), want.get(i)) for i in sorted(set(got) | set(want)) if got.get(i) != want.get(i)][:5]
    return "ok %d entries" % len(got)


def case_k_up_to_32(B):
    reads = parity_input(31, True)
    for k, m, b in ((31, 15, 14), (31, 11, 11)):
        sums = []
        for mode in ("reference", "full"):
            with B.BriskHip(k, m, b, minimizer_mode=mode) as ix:
                ix.insert_reads(reads)
                sums.append(ix.checksum())
        assert sums[0] == sums[1] and sums[0][0] > 0, (k, m, b, sums)
    return "ok"


def host_counts(reads, k):
    return Counter(c for r in reads for c in MR.canonical_kmers(r, k))


def case_one_entry(B):
    reads = MR.tie_free_reads(K, M)
    host = host_counts(reads, K)
    hist = np.bincount(np.array(list(host.values())) % 256, minlength=256)
    with B.BriskHip(K, M, B_, minimizer_mode="full") as ix, B.BriskHip(K, M, B_) as ref:
        ix.insert_reads(reads)
        ref.insert_reads(reads)
        n_full, n_ref = ix.stats()["nb_kmers"], ref.stats()["nb_kmers"]
        assert n_full == len(host), (n_full, len(host))
        assert np.array_equal(ix.count_spectrum(), hist.astype(np.uint64))
        assert n_ref > n_full, (n_ref, n_full)
    return "ok %d entries in full mode, %d in reference mode, %d canonical k-mers" % (n_full, n_ref, len(host))


def case_strand(B):
    reads = MR.tie_free_reads(K, M)
    back = [MR.revcomp(r) for r in reads]
    with B.BriskHip(K, M, B_, minimizer_mode="full") as fwd, B.BriskHip(K, M, B_, minimizer_mode="full") as rev:
        fwd.insert_reads(reads)
        rev.insert_reads(back)
        assert fwd.checksum() == rev.checksum() and fwd.checksum()[0] > 0
        counts, found, base = fwd.get_kmers(back)
        assert int(base[-1]) == sum(len(r) - K + 1 for r in reads) and found.all(), int((~found).sum())
        host = host_counts(reads, K)
        want = [host[c] % 256 for r in back for c in MR.canonical_kmers(r, K)]
        assert counts.tolist() == want
    return "ok %d slots" % int(base[-1])


def case_windows(B):
    rng = random.Random(4)
    g = "".join(rng.choice("ACGT") for _ in range(6000))
    reads = [g[p:p + 150] for p in (rng.randrange(len(g) - 150) for _ in range(400))]
    assert MR.windows_tie_free(reads, K, M)
    windows = [r[o:o + 2 * K - 1] for r, o in ((r, rng.randrange(150 - (2 * K - 1) + 1)) for r in reads)]
    whole = {}
    for mode in ("full", "reference"):
        with B.BriskHip(K, M, B_, minimizer_mode=mode) as ix:
            ix.insert_reads(reads)
            ix.insert_reads(reads)
            counts, found, base = ix.get_kmers(windows)
            whole[mode] = sum(bool(found[int(base[i]):int(base[i + 1])].all()) for i in range(len(windows)))
    assert whole["full"] == 400, whole
    assert whole["reference"] < 400, whole
    return "ok whole windows: %d of 400 in full mode, %d in reference mode" % (whole["full"], whole["reference"])


def case_correction(B):
    from correct_reference import code_of
    from test_correct import planted_reads
    _, clean, bad, where = planted_reads(K)
    n = {}
    for mode in ("reference", "full"):
        with B.BriskHip(K, M, B_, minimizer_mode=mode) as ix:
            ix.insert_reads(clean + clean)
            rows, st = ix.correct_reads(bad, 2, K)
            n[mode] = len(rows)
            assert st["n_corrected"] == len(rows)
            if mode == "full":
                for row in rows:
                    r = int(row["read"])
                    assert int(row["pos"]) == where[r] and int(row["to"]) == code_of(clean[r][where[r]]) and int(row["from"]) == code_of(bad[r][where[r]]), row
    assert n["full"] >= n["reference"], n
    return "ok corrections of %d planted substitutions: %d on the full-mode index, %d on the reference-mode index" % (len(bad), n["full"], n["reference"])


def case_plumbing(B):
    reads = MR.tie_free_reads(K, M)
    assert MR.windows_tie_free(reads, K, M + 2)
    done = 0
    with tempfile.TemporaryDirectory() as tmp, B.BriskHip(K, M, B_, minimizer_mode="full") as ix, B.BriskHip(K, M, B_) as ref:
        assert ix.layout["minimizer_mode"] == 1 and ix.minimizer_mode == "full" and ref.layout["minimizer_mode"] == 0 and ref.minimizer_mode == "reference"
        ix.insert_reads(reads)
        ref.insert_reads(reads)
        # save / open: the mode and the digest travel
        path = os.path.join(tmp, "full.snap")
        ix.save(path)
        assert open(path, "rb").read(120)[116] == 1 and B.snapshot_info(path)["minimizer_mode"] == 1
        with B.BriskHip.open(path) as again:
            assert again.minimizer_mode == "full" and again.checksum() == ix.checksum()
        with B.BriskHip(K, M, B_) as other:  # load into the other mode
            try:
                other.load(path)
                raise AssertionError("a full-mode snapshot went into a reference-mode index")
            except B.BriskHipError as e:
                assert e.code in (EINVAL, EFORMAT) and "minimizer_mode" in str(e), str(e)
            assert other.checksum()[0] == 0
        old = os.path.join(tmp, "ref.snap")
        ref.save(old)
        assert open(old, "rb").read(120)[116] == 0
        with B.BriskHip.open(old) as again:
            assert again.minimizer_mode == "reference" and again.checksum() == ref.checksum()
        done += 1
        # two handles in one operation
        for call in (lambda: ix.merge(ref), lambda: ref.merge(ix), lambda: ix.intersect(ref), lambda: ix.subtract(ref), lambda: ix.compare(ref), lambda: ix.joint_spectrum(ref)):
            try:
                call()
                raise AssertionError("mixed modes went through")
            except B.BriskHipError as e:
                assert e.code == EINVAL and "minimizer_mode" in str(e), str(e)
        with B.BriskHip(K, M + 2, B_ + 2) as fresh:
            try:
                ix.reallocate_into(fresh)
                raise AssertionError("reallocate into the other mode went through")
            except B.BriskHipError as e:
                assert e.code == EINVAL and "minimizer_mode" in str(e), str(e)
        done += 1
        # reallocate, full to full: the identities a full-mode scan gives at the new m
        with B.BriskHip(K, M + 2, B_ + 2, minimizer_mode="full") as fresh:
            ix.reallocate_into(fresh)
            want = {i: c % 256 for i, c in MR.index_of(reads, K, M + 2, True).items()}
            assert entries(fresh) == want
        done += 1
    # brisk_hip_scan_sequence follows the handle's mode (entry-id handles may be created in full mode)
    seqs = parity_input(K, False)[:40] + [r for r in MR.parity_reads() if len(r) >= K][:12]
    with B.BriskHip(K, M, B_, entry_ids=True, minimizer_mode="full") as ix:
        for s in seqs:
            ret, cnt, lo, hi, idx = ix.scan_sequence(s)
            e = MR.enumerate_read(s, K, M, True)
            assert (ret.tolist(), cnt.tolist(), list(zip(lo.tolist(), hi.tolist(), idx.tolist()))) == (e.rets, e.cuts, e.kmers), s
    done += 1
    # brisk_count
    import oracle
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(exe + ".cpp"):
        B.build_apps()
    fa = os.path.join(ROOT, "tests", "golden", "test.fa")
    fasta = oracle.fasta_sequences(open(fa).read())
    want = MR.index_of([s for s in fasta if len(s) >= K], K, M, True)
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "dump.txt")
        p = subprocess.run([exe, "--bulk", fa, str(K), str(M), str(B_), dump, "--full-minimizers"], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        n_lines = sum(1 for _ in open(dump))
        assert n_lines == len(want) and ("nb_kmers %d " % len(want)) in p.stdout, (n_lines, len(want), p.stdout[-500:], p.stderr[-500:])
        p = subprocess.run([exe, "--facade", fa, str(K), str(M), str(B_), "--full-minimizers"], capture_output=True, text=True, timeout=600)
        assert p.returncode == 2 and "--bulk only" in p.stderr
    done += 1
    return "ok %d" % done


def case_sharded(B):
    import sharded_job as S
    import torch
    from brisk_amd.exchange import uniform_cuts
    reads = parity_input(K, False)
    with B.BriskHip(K, M, B_, minimizer_mode="full") as one:
        one.insert_reads(reads)
        whole = one.checksum()
    owners = [B.BriskHip(K, M, B_, owner_rank=r, n_owners=2, minimizer_mode="full") for r in range(2)]
    try:
        job = SimpleNamespace(owners=owners, layout=owners[0].layout, b=B_, cuts=uniform_cuts(owners[0].layout["part_bits"], 2), records=None)
        inbox, _ = S.scan_all(job, reads)
        W = owners[0].record_words
        for ix, recv in zip(owners, inbox):
            torch.cuda.synchronize()
            n = recv.numel() // W
            ix.insert_records(recv.data_ptr() if n else 0, n)
            ix.sync()
        sums = [ix.checksum() for ix in owners]
    finally:
        for ix in owners:
            ix.close()
    got = (sums[0][0] + sums[1][0], sums[0][1] + sums[1][1], (sums[0][2] + sums[1][2]) % (1 << 64))
    assert got == whole and sums[0][0] > 0 and sums[1][0] > 0, (sums, whole)
    want = MR.index_of(reads, K, M, True)
    assert whole[0] == len(want) and whole[1] == sum(want.values())  # (counts stay below 256 here)
    return "ok"


def all_cases():
    cases = {}
    for k, m, b in GEOMETRIES:
        for full in (True, False):
            cases["parity-k%d-m%d-b%d-%s" % (k, m, b, "full" if full else "reference")] = (lambda B, g=(k, m, b), f=full: case_parity(B, *g, f))
    cases.update({"k_up_to_32": case_k_up_to_32, "one_entry": case_one_entry, "strand": case_strand, "windows": case_windows, "correction": case_correction,
                  "plumbing": case_plumbing, "sharded": case_sharded})
    return cases


def main(argv):
    out, names = argv[0], argv[1:]
    cases = all_cases()
    B = brisk()
    results = {}
    for name in names or list(cases):
        try:
            results[name] = cases[name](B)
        except Exception:
            results[name] = traceback.format_exc()
        print(name, results[name].splitlines()[-1] if results[name] else "", flush=True)
        with open(out, "w") as f:
            json.dump(results, f)
    print("done %d" % len(results))


if __name__ == "__main__":
    main(sys.argv[1:])
