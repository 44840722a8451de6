"""The device side of tests/test_graph.py, run in a child process: every case of the de Bruijn adjacency calls against the host
definitions in brisk_amd/hipapi.py (neighbour_strings, adjacency_from_slots, degree_spectrum_from_adjacency, graph_figures), against a
plain Python dictionary of the reads' canonical k-mers, or against an index built afresh from what must be left.

    python tests/graph_worker.py OUT.json [case ...]
    python tests/graph_worker.py --rounds OUT.npz        (a child of the `rounds` case, under its own BRISK_GRAPH_BATCH)

Runs the named cases (default: all), writes {case: "ok ..." or the failure's traceback} to OUT.json and prints "done <n>"."""
import json
import os
import random
import subprocess
import sys
import tempfile
import traceback
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import minimizer_reference as MR  # noqa: E402

EINVAL, ECAPACITY = 1, 5
# (k, m, b, minimizer_mode): odd k (an entry's eight reads are not whole words) and even k, the first k with a `hi` word, 9-byte
# (k31, k32) and 17-byte entries, a non-zero shift (b = 14); b as the other small-geometry tests take it
GEOMETRIES = [(31, 15, 14, "reference"), (32, 15, 14, "reference"), (33, 17, 8, "full"), (63, 21, 14, "full"), (63, 31, 12, "full")]
MIN_COUNTS = (0, 1, 2, 255)
ISOLATED_AND_DEAD_ENDS = [(0, 0), (0, 1), (1, 0)]


def brisk():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


def name_of(k, m, b, mode):
    return "k%d-m%d-b%d-%s" % (k, m, b, mode)


def genome_reads(k, m, genome=3000, n=450, L=100):
    """100-nt reads at 15x of a 3 kb random genome, either strand, seeded so that no k-mer window holds two equal canonical m-mers"""
    reads = MR.tie_free_reads(k, m, n=n, L=L, genome=genome)
    assert MR.windows_tie_free(reads, k, m)
    return reads


def random_tie_free(k, m, length, seed):
    for s in range(seed, seed + 50):
        rng = random.Random(s)
        x = "".join(rng.choice("ACGT") for _ in range(length))
        if MR.windows_tie_free([x], k, m):
            return x
    raise AssertionError("no tie-free seed")


def host_counts(reads, k):
    return Counter(c for r in reads for c in MR.canonical_kmers(r, k))


def yardstick(B, ix, min_counts):
    """adjacency_from_slots(get_kmers(neighbour_strings(enumerate()))) for every min_count: one enumerate, one get_kmers"""
    lo, hi, idx, cnt = ix.enumerate()
    strings = B.neighbour_strings(lo, hi, ix.k)
    counts, found, base = ix.get_kmers(strings)
    assert int(base[-1]) == 8 * len(lo)
    return {mc: B.adjacency_from_slots(counts, found, mc) for mc in min_counts}, strings, cnt


def check_composition(B, ix, min_counts=MIN_COUNTS):
    want, strings, cnt = yardstick(B, ix, min_counts)
    for mc in min_counts:
        got = ix.adjacency(mc)
        assert got.dtype == np.uint8 and len(got) == len(cnt), (len(got), len(cnt))
        bad = np.nonzero(got != want[mc])[0]
        assert len(bad) == 0, (mc, len(bad), [(int(i), int(got[i]), int(want[mc][i])) for i in bad[:5]])
    return want, strings, cnt


def case_composition(B, k, m, b, mode):
    reads = genome_reads(k, m)
    with B.BriskHip(k, m, b, minimizer_mode=mode) as ix:
        ix.insert_reads(reads)
        ix.insert_reads(reads[:150])  # (more of the counts differ)
        want, _, cnt = check_composition(B, ix)
        assert want[0].any() and (want[0] != want[2]).any() and not want[255].any()
    return "ok %d entries" % len(cnt)


def case_composition_count_modes(B):
    k, m, b, mode = GEOMETRIES[0]
    reads = genome_reads(k, m)
    n = {}
    for count_mode in ("wrap", "saturate"):
        with B.BriskHip(k, m, b, count_mode=count_mode) as ix:
            for _ in range(16):  # 15x sixteen times: a k-mer seen 16 times in the reads wraps to 0, or is held at 255
                ix.insert_reads(reads)
            sp = ix.count_spectrum()
            assert (sp[0] > 0) == (count_mode == "wrap") and (count_mode == "wrap" or sp[255] > 0), sp
            want, _, cnt = check_composition(B, ix)
            n[count_mode] = int((want[0] != want[1]).sum())
    assert n["wrap"] > 0 and n["saturate"] == 0, n  # a present entry with count 0 is a neighbour at min_count 0 only
    return "ok"


def case_composition_ties(B):
    """homopolymers and periodic reads: ties abound and there is no host truth -- the lookup decides, the composition must hold"""
    total = 0
    for k, m, b, mode in (GEOMETRIES[0], GEOMETRIES[3]):
        reads = [r for r in MR.parity_reads() if len(r) >= k] + ["A" * (k + 5), "C" * k, "AC" * k, "ACG" * k, "AACCTTGG" * 20]
        with B.BriskHip(k, m, b, minimizer_mode=mode) as ix:
            ix.insert_reads(reads)
            _, _, cnt = check_composition(B, ix)
            total += len(cnt)
    return "ok %d entries" % total


def case_composition_reference_k63(B):
    k, m, b = 63, 21, 14
    reads = genome_reads(k, m)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(reads)
        want, _, cnt = check_composition(B, ix)
    return "ok %d entries, %d of them with a neighbour found" % (len(cnt), int((want[0] != 0).sum()))


def case_truth(B, k, m, b, mode):
    reads = genome_reads(k, m)
    every = reads + reads[:150]
    host = host_counts(every, k)
    assert max(host.values()) < 256
    with B.BriskHip(k, m, b, minimizer_mode=mode) as ix:
        ix.insert_reads(reads)
        ix.insert_reads(reads[:150])
        lo, hi, idx, cnt = ix.enumerate()
        assert len(lo) == len(host), (len(lo), len(host))  # one canonical k-mer, one entry
        strings = B.neighbour_strings(lo, hi, k)
        mult = np.array([host.get(min(s, MR.revcomp(s)), -1) for s in (x.decode() for x in strings)], np.int64).reshape(-1, 8)
        n_set = 0
        for mc in MIN_COUNTS:
            want = ((mult >= mc) << np.arange(8)).sum(axis=1).astype(np.uint8)  # (-1: absent, below every threshold)
            got = ix.adjacency(mc)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (mc, len(bad), [(int(i), int(got[i]), int(want[i])) for i in bad[:5]])
            n_set += int(np.unpackbits(got).sum())
    return "ok %d entries, %d bits set over the thresholds" % (len(lo), n_set)


def figures(B, k, m, b, mode, reads, min_count=0):
    assert MR.windows_tie_free(reads, k, m)
    with B.BriskHip(k, m, b, minimizer_mode=mode) as ix:
        ix.insert_reads(reads)
        sp = ix.degree_spectrum(min_count)
        assert int(sp.sum()) == ix.stats()["nb_kmers"]
        return B.graph_figures(sp), sp


def case_crafted(B):
    done = 0
    for k, m, b, mode in (GEOMETRIES[0], GEOMETRIES[1], GEOMETRIES[3]):
        # one read of length L: L - k - 1 simple nodes and two dead ends
        L = 150
        one = random_tie_free(k, m, L, 11)
        f, sp = figures(B, k, m, b, mode, [one])
        assert f == dict(nodes=L - k + 1, edge_ends=2 * (L - k), isolated=0, dead_ends=2, simple=L - k - 1, branching=0, below=0), f
        assert sp[B.degree_class(0, 1)] + sp[B.degree_class(1, 0)] == 2
        # two reads that share a prefix longer than k and then diverge: exactly one node with a side of degree 2
        stem = random_tie_free(k, m, k + 20, 21)
        arm_a, arm_b = random_tie_free(k, m, 2 * k, 31), random_tie_free(k, m, 2 * k, 41)
        arm_b = ("A" if arm_a[0] != "A" else "C") + arm_b[1:]
        f, sp = figures(B, k, m, b, mode, [stem + arm_a, stem + arm_b])
        assert f["branching"] == 1 and sp[B.degree_class(1, 2)] + sp[B.degree_class(2, 1)] == 1 and f["dead_ends"] == 3 and f["isolated"] == 0, (f, sp)
        assert f["nodes"] == (20 + 1) + 2 * 2 * k and f["simple"] == f["nodes"] - 4
        # a read of exactly k nucleotides unrelated to the rest: one isolated node
        f, sp = figures(B, k, m, b, mode, [one, random_tie_free(k, m, k, 51)])
        assert f["isolated"] == 1 and f["dead_ends"] == 2 and f["simple"] == L - k - 1 and f["nodes"] == L - k + 2, f
        # a circular sequence read once round plus k - 1: all nodes simple, no dead end
        N = 200
        for seed in range(61, 111):
            ring = random_tie_free(k, m, N, seed)
            if MR.windows_tie_free([ring + ring[:k - 1]], k, m):
                break
        f, sp = figures(B, k, m, b, mode, [ring + ring[:k - 1]])
        assert f == dict(nodes=N, edge_ends=2 * N, isolated=0, dead_ends=0, simple=N, branching=0, below=0), f
        # the threshold: the path's k-mers seen once, a part of it twice -- at min_count 2 the part is the graph, the rest is below
        f, sp = figures(B, k, m, b, mode, [one, one[20:20 + k + 9]], min_count=2)
        assert f == dict(nodes=10, edge_ends=18, isolated=0, dead_ends=2, simple=8, branching=0, below=L - k + 1 - 10), f
        done += 1
    return "ok %d geometries" % done


def case_forms(B):
    import torch
    k, m, b, mode = GEOMETRIES[3]
    reads = genome_reads(k, m)
    with B.BriskHip(k, m, b, minimizer_mode=mode) as ix:
        ix.insert_reads(reads)
        ix.insert_reads(reads[:150])
        lo, hi, idx, cnt = ix.enumerate()
        n = len(lo)
        assert ix.stats()["nb_kmers"] == n
        for mc in (0, 2):
            adj = ix.adjacency(mc)
            buf = torch.full((n + 64,), 0xAA, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            assert ix.adjacency_device(buf.data_ptr(), n + 64, mc) == n
            host = buf.cpu().numpy()
            assert np.array_equal(host[:n], adj) and (host[n:] == 0xAA).all()
            sp = ix.degree_spectrum(mc)
            assert np.array_equal(sp, B.degree_spectrum_from_adjacency(adj, cnt, mc)), (sp, mc)
            assert int(sp.sum()) == n and (mc != 0 or sp[25] == 0)
        buf = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        try:
            ix.adjacency_device(buf.data_ptr(), n - 1, 0)
            raise AssertionError("cap one short went through")
        except B.BriskHipError as e:
            assert e.code == ECAPACITY and str(n) in str(e), str(e)
        assert (buf.cpu().numpy() == 0xAA).all()
    with B.BriskHip(k, m, b, minimizer_mode=mode) as empty:
        assert len(empty.adjacency()) == 0 and not empty.degree_spectrum().any() and empty.prune_degrees(ISOLATED_AND_DEAD_ENDS) == 0
    return "ok %d entries" % n


# ---- rounds
def cluster_reads(B, k, m, b):
    """100 reads of exactly k nucleotides around one m-mer that is the minimizer of (nearly) all of them -- so that one partition
    holds more than 64 entries in a directory that is otherwise almost empty.  The m-mer is found by trying: the order is the library's."""
    rng = random.Random(5)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    left = (k - m) // 2
    with B.BriskHip(k, m, b) as probe:
        cands = [rnd(m) for _ in range(4096)]
        keys = probe.debug_order_keys([int(MR_pack(c)) for c in cands])
    for i in np.argsort(keys)[:40]:
        core = cands[int(i)]
        reads = [rnd(left) + core + rnd(k - m - left) for _ in range(100)]
        with B.BriskHip(k, m, b) as ix:
            ix.insert_reads(reads)
            lo, hi, idx, cnt = ix.enumerate()
        if len(lo) and Counter(idx.tolist()).most_common(1)[0][1] > 80:
            return reads
    raise AssertionError("no m-mer made a partition of more than 64 entries")


def MR_pack(s):
    v = 0
    for ch in s:
        v = (v << 2) | "ACTG".index(ch)
    return v


def rounds_input(B):
    k, m, b, mode = GEOMETRIES[0]
    return (k, m, b), genome_reads(k, m, genome=2000, n=300) + cluster_reads(B, k, m, b)


def rounds_bytes(B):
    (k, m, b), reads = rounds_input(B)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(reads)
        # (storage order inside a partition is the insert's business: rows are compared in the order of their identities)
        lo, hi, idx, cnt = ix.enumerate()
        order = np.lexsort((idx, lo, hi))
        want, _, _ = check_composition(B, ix, (0, 2))  # under this process' batch
        out = {"adj%d" % mc: ix.adjacency(mc) for mc in (0, 2)}
        assert all(np.array_equal(out["adj%d" % mc], want[mc]) for mc in (0, 2))
        out["spectrum"] = ix.degree_spectrum(1)
        assert np.array_equal(out["spectrum"], B.degree_spectrum_from_adjacency(ix.adjacency(1), cnt, 1))
        # the directory: every partition's size
        sizes = ix.debug_directory(np.arange(1 << ix.layout["part_bits"], dtype=np.uint32))[0]
        out["sizes"] = sizes[sizes > 0]
        first, last = np.nonzero(sizes)[0][[0, -1]]
        out["empty_between"] = np.array([int((sizes[first:last + 1] == 0).sum())])
        before = ix.enumerate()
        ix.prune_degrees(ISOLATED_AND_DEAD_ENDS + [(1, 2), (2, 1)])
        out["after_prune"] = np.array(ix.checksum(), np.uint64)
        out["mask_rows"] = np.isin(classes_of(out["adj0"]), [0, 1, 5, 7, 11])
        assert len(before[0]) - int(out["mask_rows"].sum()) == ix.stats()["nb_kmers"]
        for name in ("adj0", "adj2", "mask_rows"):
            out[name] = out[name][order]
    return out


def case_rounds(B):
    mine = rounds_bytes(B)
    assert "BRISK_GRAPH_BATCH" not in os.environ
    assert mine["sizes"].max() > 64 and mine["empty_between"][0] > 0, (mine["sizes"].max(), mine["empty_between"])
    assert (mine["sizes"] <= 5).sum() > 10  # rounds of several small partitions at batch 5, besides the ones that go alone
    with tempfile.TemporaryDirectory() as tmp:
        for batch in ("1", "5"):
            out = os.path.join(tmp, "rounds%s.npz" % batch)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", out], env=dict(os.environ, BRISK_GRAPH_BATCH=batch), capture_output=True, text=True,
                               timeout=600)
            assert p.returncode == 0 and os.path.exists(out), (batch, p.returncode, p.stdout[-1000:], p.stderr[-3000:])
            theirs = np.load(out)
            for name in mine:
                assert np.array_equal(mine[name], theirs[name]), (batch, name)
    return "ok %d entries, the largest partition %d, %d empty partitions between the first and the last" % (len(mine["adj0"]), mine["sizes"].max(), mine["empty_between"][0])


# ---- prune_degrees
def entry_strings(lo, hi, k):
    out = []
    for a, c in zip(lo.tolist(), hi.tolist()):
        v = (c << 64) | a
        out.append("".join("ACTG"[(v >> (2 * (k - 1 - j))) & 3] for j in range(k)))
    return out


def classes_of(adj):
    pop = np.array([bin(i).count("1") for i in range(16)])
    return 5 * pop[adj >> 4] + pop[adj & 15]


def case_prune_degrees(B, k, m, b, mode):
    reads = genome_reads(k, m)
    lonely = [random_tie_free(k, m, k, 300 + i) for i in range(3)]           # isolated nodes
    path3, path2 = random_tie_free(k, m, k + 2, 400), random_tie_free(k, m, k + 1, 500)  # a - b - c, and two dead ends that touch
    heavy = random_tie_free(k, m, k, 600)
    every = reads + reads[:150] + lonely + [path3, path2] + [heavy] * 3
    assert MR.windows_tie_free(every, k, m)
    min_count, max_count = 1, 2
    mask_pairs = ISOLATED_AND_DEAD_ENDS
    with B.BriskHip(k, m, b, minimizer_mode=mode) as ix, B.BriskHip(k, m, b, minimizer_mode=mode) as fresh:
        ix.insert_reads(every)
        lo, hi, idx, cnt = ix.enumerate()
        strings = entry_strings(lo, hi, k)
        adj = ix.adjacency(min_count)
        sums = ix.checksum()
        # empty mask, and a window that holds no entry: nothing goes, nothing changes
        assert ix.prune_degrees(0, min_count, max_count) == 0 and ix.prune_degrees([], 0, 255) == 0
        assert ix.prune_degrees(mask_pairs, 200, 201) == 0 and ix.prune_degrees(mask_pairs, 300, 400) == 0
        assert ix.checksum() == sums and all(np.array_equal(x, y) for x, y in zip(ix.enumerate(), (lo, hi, idx, cnt)))
        # rows
        gone = np.isin(classes_of(adj), [B.degree_class(*p) for p in mask_pairs]) & (cnt >= min_count) & (cnt <= max_count)
        by_string = dict(zip(strings, gone.tolist()))
        canon = lambda s: by_string[s] if s in by_string else by_string[MR.revcomp(s)]
        p3 = [path3[i:i + k] for i in range(3)]
        assert [canon(s) for s in p3] == [True, False, True]  # the middle node had two neighbours when the call began
        assert [canon(path2[i:i + k]) for i in range(2)] == [True, True] and all(canon(s) for s in lonely)
        assert not canon(heavy)  # isolated, but seen three times: outside the window
        removed = ix.prune_degrees(mask_pairs, min_count, max_count)
        assert removed == int(gone.sum()) and removed >= 7, (removed, int(gone.sum()))
        after = ix.enumerate()
        for x, y in zip(after, (lo, hi, idx, cnt)):
            assert np.array_equal(x, y[~gone])
        # digest: the index built afresh from the survivors
        left = [s for s, g, c in zip(strings, gone.tolist(), cnt.tolist()) if not g for _ in range(c)]
        fresh.insert_reads(left)
        st, want = ix.stats(), fresh.stats()
        assert (st["nb_kmers"], st["nb_buckets"]) == (want["nb_kmers"], want["nb_buckets"]) and st["nb_kmers"] == len(lo) - removed, (st, want)
        assert ix.checksum() == fresh.checksum()
        # lookups
        counts, found, base = ix.get_kmers(strings)
        assert np.array_equal(found, ~gone) and np.array_equal(counts[found], cnt[~gone])
        # a removed k-mer that is inserted again starts at 1
        back = [s for s, g in zip(strings, gone.tolist()) if g][:5]
        ix.insert_reads(back)
        counts, found, base = ix.get_kmers(back)
        assert found.all() and counts.tolist() == [1] * len(back)
        assert ix.stats()["nb_kmers"] == len(lo) - removed + len(back)
    return "ok %d of %d entries removed" % (removed, len(lo))


def case_refusals(B):
    k, m, b = 31, 15, 14
    n = 0
    def refused(call, *words):
        nonlocal n
        try:
            call()
            raise AssertionError("went through: %s" % (words,))
        except B.BriskHipError as e:
            assert e.code == EINVAL and all(w in str(e) for w in words), (str(e), words)
        n += 1
    with B.BriskHip(k, m, b, owner_rank=0, n_owners=2) as shard:
        for call in (lambda: shard.adjacency_device(0, 0), lambda: shard.degree_spectrum(), lambda: shard.prune_degrees(1)):
            refused(call, "sharded", "n_owners > 1", "follow-up")
    with B.BriskHip(k, m, b, entry_ids=True) as ids:
        for call in (lambda: ids.adjacency_device(0, 0), lambda: ids.degree_spectrum(), lambda: ids.prune_degrees(1)):
            refused(call, "entry-id")
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(genome_reads(k, m)[:20])
        sums = ix.checksum()
        refused(lambda: ix.prune_degrees(1, 3, 2), "min_count > max_count")
        refused(lambda: ix.prune_degrees(1 << 25), "bit above 24")
        refused(lambda: ix.prune_degrees(0xffffffff), "bit above 24")
        assert ix.checksum() == sums
        assert ix.prune_degrees(1 << 24) == 0  # the highest class is one
    return "ok %d" % n


def case_brisk_count(B):
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(exe + ".cpp"):
        B.build_apps()
    k, m, b, mode = GEOMETRIES[3]
    reads = genome_reads(k, m)[:200] + [random_tie_free(k, m, k, 300 + i) for i in range(3)]
    with B.BriskHip(k, m, b, minimizer_mode=mode) as ix:
        ix.insert_reads(reads)
        want = {mc: ix.degree_spectrum(mc) for mc in (0, 2)}
        n_entries = ix.stats()["nb_kmers"]
    assert want[0][0] >= 3
    with tempfile.TemporaryDirectory() as tmp:
        fa, deg = os.path.join(tmp, "reads.fa"), os.path.join(tmp, "degrees.tsv")
        with open(fa, "w") as f:
            for i, r in enumerate(reads):
                f.write(">%d\n%s\n" % (i, r))
        for mc in (0, 2):
            cmd = [exe, "--bulk", fa, str(k), str(m), str(b), "--full-minimizers", "--degrees", deg] + (["--min-count", "2"] if mc else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
            lines = open(deg).read().split("\n")
            got = [int(x) for line in lines[:5] for x in line.split("\t")] + [int(lines[5].split("\t")[1])]
            assert lines[5].startswith("below\t") and got == want[mc].tolist(), (got, want[mc].tolist())
            f = B.graph_figures(want[mc])
            assert "%d nodes, %d edge ends, %d isolated, %d dead ends, %d simple, %d branching" % (f["nodes"], f["edge_ends"], f["isolated"], f["dead_ends"], f["simple"],
                                                                                              f["branching"]) in p.stderr, p.stderr[-500:]
        p = subprocess.run([exe, "--bulk", fa, str(k), str(m), str(b), "--full-minimizers", "--prune-degrees", "0:0"], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        assert "prune-degrees 0:0: %d entries removed" % int(want[0][0]) in p.stderr and ("nb_kmers %d " % (n_entries - int(want[0][0]))) in p.stdout, (p.stderr[-500:], p.stdout[-300:])
        p = subprocess.run([exe, "--bulk", fa, str(k), str(m), str(b), "--prune-degrees", "0:5"], capture_output=True, text=True, timeout=600)
        assert p.returncode == 2 and "0..4" in p.stderr
        p = subprocess.run([exe, "--facade", fa, str(k), str(m), str(b), "--degrees", deg], capture_output=True, text=True, timeout=600)
        assert p.returncode == 2 and "--bulk only" in p.stderr
        p = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
        assert "--degrees FILE" in p.stdout and "--prune-degrees L:R" in p.stdout
    return "ok"


def all_cases():
    cases = {}
    for g in GEOMETRIES:
        cases["composition-" + name_of(*g)] = lambda B, g=g: case_composition(B, *g)
        cases["truth-" + name_of(*g)] = lambda B, g=g: case_truth(B, *g)
    for g in (GEOMETRIES[0], GEOMETRIES[2], GEOMETRIES[3]):
        cases["prune_degrees-" + name_of(*g)] = lambda B, g=g: case_prune_degrees(B, *g)
    cases.update({"composition-count_modes": case_composition_count_modes, "composition-ties": case_composition_ties, "composition-reference_k63": case_composition_reference_k63,
                  "crafted": case_crafted, "forms": case_forms, "rounds": case_rounds, "refusals": case_refusals, "brisk_count": case_brisk_count})
    return cases


def main(argv):
    if argv[0] == "--rounds":
        np.savez(argv[1], **rounds_bytes(brisk()))
        return
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
