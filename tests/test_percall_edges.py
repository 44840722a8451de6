"""GPU: the per-call (entry-id) path under the C++ facade -- brisk_hip_scan_sequence, brisk_hip_upsert_kmers, brisk_hip_find_kmers,
brisk_hip_enumerate_ids: k_scan in sequence mode, k_expand_records, k_upsert, k_lookup and k_enumerate with ids -- at the geometries
where the key layout, the record and the scan change their code path (tests/geometry_edges.py).  key_of_kmer restates the bulk
path's key construction by hand, and scan_sequence runs under parameters of its own, without the class bits: this is where a second
copy of the layout code would go wrong unseen.  Expected values come from tests/percall_reference.py alone: the oracle's enumerator
stream and the protocol replayed in Python.  Every test first asserts that the library lays the row out as the formula says."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import geometry_edges as G
import oracle
import percall_reference as P

pytestmark = pytest.mark.gpu

EINVAL = 1
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
ROWS = pytest.mark.parametrize("r", G.TABLE, ids=[G.row_id(r) for r in G.TABLE])
FACADE_ROWS = [r for r in G.TABLE if not r.part_bits and (r.k, r.m, r.b) in ((33, 11, 4), (34, 11, 4), (63, 21, 2), (63, 5, 2), (33, 31, 14), (12, 5, 1))]


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


def handle(B, r):
    ix = B.BriskHip(r.k, r.m, r.b, entry_ids=True, **G.opts(r))
    G.check_library_layout(r, ix.layout)
    return ix


def check_stream(ix, rp, what):
    """scan_sequence of every sequence: the enumerator's returned minimizer values, vector lengths, lo, hi and minimizer_idx, in
    sequence order; nothing for a sequence shorter than k"""
    for s, want in zip(rp.seqs, rp.streams):
        got = ix.scan_sequence(s)
        assert len(got) == 5
        for name, a, c in zip(("ret", "n", "lo", "hi", "idx"), got, want):
            assert a.dtype == c.dtype and np.array_equal(a, c), (what, name, len(s), s[:24])
        if len(s) < rp.k:
            assert len(got[0]) == 0 and len(got[2]) == 0


def fill(ix, rp, what, after_vector=None):
    """every vector through upsert_kmers: exactly the replay's (ids, newly), and find_kmers of the vector right after gives the ids"""
    for vi, v in enumerate(rp.vectors):
        ids, newly = ix.upsert_kmers(v.lo, v.hi, v.idx)
        assert np.array_equal(ids, v.ids) and np.array_equal(newly, v.newly), (what, "upsert", vi, ids.tolist(), v.ids.tolist(), newly.tolist(), v.newly.tolist())
        assert np.array_equal(ix.find_kmers(v.lo, v.hi, v.idx), v.ids), (what, "find after upsert", vi)
        if after_vector:
            after_vector(vi)


def check_find_all(ix, rp, what, n=None, chunk=300):
    """find_kmers over entries[:n], more than 255 at a time: every entry under its id"""
    lo, hi, idx = rp.arrays(n)
    for at in range(0, len(lo), chunk):
        got = ix.find_kmers(lo[at:at + chunk], hi[at:at + chunk], idx[at:at + chunk])
        assert np.array_equal(got, np.arange(at, min(at + chunk, len(lo)), dtype=np.uint32)), (what, "find_kmers over all entries", at)


def check_end_state(O, ix, rp, r, what, n=None, data=None, count=None):
    """enumerate_ids joined with the host's DATA is the oracle's dump; stats() its nb_kmers and nb_buckets.  n, data: the first n
    entries only, with this DATA; count: O.count of the same input (else of the replay's sequences)"""
    lo, hi, idx, ids = ix.enumerate_ids()
    n = len(rp.entries) if n is None else n
    data = rp.data if data is None else data
    assert sorted(ids.tolist()) == list(range(n)), (what, "ids are dense")
    assert oracle.multiset_lines(lo, hi, idx, [data[i] for i in ids.tolist()], r.k) == rp.lines(n, data), (what, "enumerate_ids")
    st = ix.stats()
    if count is None and n == len(rp.entries):
        count = P.oracle_count(O, r, rp.seqs)
    if count is not None:
        assert rp.lines(n, data) == count[0]
        assert (st["nb_kmers"], st["nb_buckets"]) == count[1:], (what, "stats")
    assert st["nb_kmers"] == n, (what, "nb_kmers")
    return lo, hi, idx, ids


@ROWS
def test_stream(B, O, r):
    with handle(B, r) as ix:
        check_stream(ix, P.replay(O, r), G.row_id(r))
        assert ix.stats()["nb_kmers"] == 0


@ROWS
def test_upsert_find_enumerate(B, O, r):
    rp, what = P.replay(O, r), G.row_id(r)
    lo, hi, idx = rp.arrays()
    with handle(B, r) as ix:
        assert (ix.find_kmers(lo[:300], hi[:300], idx[:300]) == P.ABSENT).all(), (what, "find_kmers on a fresh handle")
        fill(ix, rp, what)
        check_find_all(ix, rp, what)
        for lo2, hi2, idx2, want in P.flipped(rp, O, r):
            assert np.array_equal(ix.find_kmers(lo2, hi2, idx2), want), (what, "find_kmers of one-bit neighbours")
        check_end_state(O, ix, rp, r, what)
        ix.clear()
        assert ix.stats()["nb_kmers"] == 0 and len(ix.enumerate_ids()[0]) == 0
        assert (ix.find_kmers(lo[:300], hi[:300], idx[:300]) == P.ABSENT).all(), (what, "find_kmers after clear")
        fill(ix, rp, (what, "second fill"))  # ids from 0 again
        check_find_all(ix, rp, (what, "second fill"))
        check_end_state(O, ix, rp, r, (what, "second fill"))


@pytest.mark.parametrize("r", [G.TABLE[0], G.TABLE[7]], ids=[G.row_id(G.TABLE[0]), G.row_id(G.TABLE[7])])
def test_refusals_leave_the_handle_as_it_was(B, O, tmp_path, r):
    """what an entry-id index does not do is refused with EINVAL, and so are a minimizer_idx beyond k - m and more than 255 k-mers in
    one upsert; a one-word and a two-word row"""
    rp, what = P.replay(O, r), G.row_id(r)
    with handle(B, r) as ix, B.BriskHip(r.k, r.m + 2, r.b + 2) as other:
        fill(ix, rp, what)
        before = [a.copy() for a in check_end_state(O, ix, rp, r, what)]
        v = max(rp.vectors, key=lambda v: len(v.ids))
        bad_idx = v.idx.copy()
        bad_idx[len(bad_idx) // 2] = r.k - r.m + 1
        many = np.resize(v.lo, 256), np.resize(v.hi, 256), np.resize(v.idx, 256)
        for call in (lambda: ix.insert_reads(rp.seqs[:2]), lambda: ix.get_kmers(rp.seqs[:2]), lambda: ix.prune(2), lambda: ix.save(tmp_path / "no.snap"),
                     lambda: ix.reallocate_into(other), lambda: ix.upsert_kmers(v.lo, v.hi, bad_idx), lambda: ix.upsert_kmers(*many)):
            with pytest.raises(B.BriskHipError) as e:
                call()
            assert e.value.code == EINVAL
        assert not os.path.exists(tmp_path / "no.snap") and other.checksum() == (0, 0, 0)
        after = check_end_state(O, ix, rp, r, what)
        order_b, order_a = np.argsort(before[3]), np.argsort(after[3])
        assert all(np.array_equal(x[order_b], y[order_a]) for x, y in zip(before, after))
        check_find_all(ix, rp, what)
        ids, newly = ix.upsert_kmers(v.lo, v.hi, v.idx)  # and it still takes a vector: all found
        assert np.array_equal(ids, v.ids) and not newly.any()


# ---- the C++ facade ------------------------------------------------------------------------------------------------------------
def _facade(tmp_path, r, seqs, name, env=None):
    import brisk_amd
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe):
        brisk_amd.build_apps()
    fa, dump = str(tmp_path / "reads.fa"), str(tmp_path / name)
    with open(fa, "w") as f:
        f.write("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    p = subprocess.run([exe, "--facade", fa, str(r.k), str(r.m), str(r.b), dump], capture_output=True, text=True, timeout=300,
                       env=dict({n: v for n, v in os.environ.items() if not n.startswith("BRISK_") or n == "BRISK_HIP_LIB"}, **(env or {})))
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, sorted(l for l in open(dump).read().split("\n") if l)


@pytest.mark.parametrize("r", FACADE_ROWS, ids=[G.row_id(r) for r in FACADE_ROWS])
def test_facade_counts_the_rows_reads(O, tmp_path, r):
    """Brisk<uint8_t> over the per-call C-ABI, as apps/counter.cpp drives it: brisk_count --facade on the row's reads"""
    rp = P.replay(O, r)
    lines, nb_kmers, nb_buckets = P.oracle_count(O, r, rp.seqs)
    stdout, dump = _facade(tmp_path, r, rp.seqs, "dump.txt")
    assert stdout.split() == ["nb_kmers", str(nb_kmers), "nb_buckets", str(nb_buckets), "sum_counts", str(sum(rp.data))]
    assert dump == lines == rp.lines()


def test_facade_reallocate_at_a_one_word_key(O, tmp_path):
    """Brisk::reallocate behind the facade at (33, 11, 4) -> (33, 13, 6), a 64-bit key with classes to a 60-bit one without: every
    entry's DATA arrives under its new identity (checked as test_reallocate.test_facade_reallocate_carries_the_data_over does: entries
    that merge keep the DATA of any one of them).  Every k-mer of this row yields exactly one (k-mer, minimizer_idx) at m + 2."""
    from test_reallocate import _lines_to_counter, _one_kmer
    r = G.TABLE[0]
    assert (r.k, r.m, r.b) == (33, 11, 4) and G.layout(r.k, r.m + 2, r.b + 2)["key_bits"] == 60
    rp = P.replay(O, r)
    stdout, after = _facade(tmp_path, r, rp.seqs, "after.txt", env={"BRISK_REALLOCATE": "1"})
    assert "reallocated k 33 m 13 b 6" in stdout
    want = {}
    for (lo, hi, _), cnt in zip(rp.entries, rp.data):
        got = _one_kmer(O, oracle.kmer2str(lo, hi, r.k), r.k, r.m + 2)
        assert len(got) == 1
        want.setdefault(got[0], set()).add(cnt)
    have = _lines_to_counter(after)
    assert set(have) == set(want)
    assert all(have[key] in want[key] for key in have)
    assert len(have) > 1000 and sum(len(v) > 1 for v in want.values()) * 10 < len(want)


# ---- BRISK_CLS_BITS, BRISK_NO_VMM, BRISK_ARENA_LIMIT: a process per environment (the library reads them when a handle is created) --------
def _worker(mode, extra_env):
    env = {n: v for n, v in os.environ.items() if not n.startswith("BRISK_") or n == "BRISK_HIP_LIB"}
    env.update(extra_env)
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(TESTS, "percall_worker.py"), mode], env=env, capture_output=True, text=True, timeout=600)
    print(f"percall_worker {mode} {extra_env}: {time.time() - t0:.0f} s")
    print(p.stdout)
    last = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
    assert p.returncode == 0 and last.startswith("ok "), (extra_env, p.stdout[-4000:], p.stderr[-6000:])
    return int(last.split()[1])


@pytest.mark.parametrize("bits", [0, 2, 3])
def test_cls_bits(bits):
    """stream, upsert / find / enumerate and stats at the class rows under every BRISK_CLS_BITS: scan_sequence still hands out whole
    vectors, and key_of_kmer's class follows the setting"""
    assert _worker("cls", {"BRISK_CLS_BITS": str(bits)}) == 3 * len(G.cls_rows())


def test_arena_growth_without_vmm():
    """BRISK_NO_VMM=1: the arena grows by copy at least twice under the per-call fill, ids survive, and a vector is resumed part-way
    (the BRISK_TRACE line of the resume path), at the sizes and k-mers tests/percall_reference.predict_growths names"""
    assert _worker("growth", {"BRISK_NO_VMM": "1", "BRISK_TRACE": "1"}) == 2 * len(P.GROWTH_ROWS)


def test_arena_limit_is_enomem_and_a_prefix():
    """BRISK_ARENA_LIMIT between the first and the second growth: the upsert that needs the second answers ENOMEM; the k-mers of its
    vector that were in stay in, under the next ids"""
    assert _worker("limit", {"BRISK_NO_VMM": "1", "BRISK_TRACE": "1"}) == 2 * len(P.GROWTH_ROWS)
