"""brisk_count --bulk with --histo / --min-count / --max-count (GPU): the histogram file equals the oracle's bincount, the dump
and the KFF file hold exactly the filtered multiset; and a command line without the options gives the dump it always gave."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kff_reader import read_kff  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
FASTA = os.path.join(GOLD, "test.fa")
K, M, B_ = 31, 11, 4


def _exe():
    import brisk_amd
    exe = os.path.join(ROOT, "brisk_amd", "apps", "brisk_count")
    if not os.path.exists(exe):
        brisk_amd.build_apps()
    return exe


def _oracle_dump(O):
    seqs = oracle.fasta_sequences(open(FASTA).read())
    h = O.index_new(K, M, B_)
    flat, offs = oracle.pack_reads(seqs)
    O.index_insert_reads(h, flat, offs)
    dump, nb_buckets = O.index_dump(h), O.index_stats(h)[1]
    O.index_free(h)
    return dump, nb_buckets


def _lines(dump, lo=0, hi=255):
    mask = (dump[3] >= lo) & (dump[3] <= hi)
    return oracle.multiset_lines(*(a[mask] for a in dump), K)


@pytest.mark.gpu
def test_histo_and_count_bounds(tmp_path, O):
    dump, _ = _oracle_dump(O)
    assert len(np.unique(dump[3])) > 1 and (dump[3] >= 2).any() and (dump[3] < 2).any()
    histo, out, kff = str(tmp_path / "histo.tsv"), str(tmp_path / "dump.txt"), str(tmp_path / "out.kff")
    # options before, between and after the positional arguments
    run = subprocess.run([_exe(), "--bulk", "--histo", histo, FASTA, str(K), str(M), str(B_), "--min-count", "2", out, kff],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    want_hist = np.bincount(dump[3], minlength=256)
    rows = [l.split("\t") for l in open(histo).read().splitlines()]
    assert [int(r[0]) for r in rows] == list(range(256)) and all(len(r) == 2 for r in rows)
    assert [int(r[1]) for r in rows] == want_hist.tolist()
    want = _lines(dump, 2, 255)
    assert open(out).read().splitlines() == want
    _, ents = read_kff(kff)
    assert sorted(f"{km} {idx} {data[0]}" for km, idx, data in ents) == want
    # nb_kmers is the whole index's, the sum is of what was dumped
    words = run.stdout.split()
    assert int(words[words.index("nb_kmers") + 1]) == len(dump[0])
    assert int(words[words.index("sum_counts") + 1]) == int(dump[3][dump[3] >= 2].astype(np.int64).sum())
    # an upper bound alone
    run = subprocess.run([_exe(), "--bulk", FASTA, str(K), str(M), str(B_), out, "--max-count", "1"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert open(out).read().splitlines() == _lines(dump, 0, 1)


@pytest.mark.gpu
def test_a_command_line_without_the_options_is_unchanged(tmp_path, O):
    dump, nb_buckets = _oracle_dump(O)
    out, kff = str(tmp_path / "dump.txt"), str(tmp_path / "out.kff")
    run = subprocess.run([_exe(), "--bulk", FASTA, str(K), str(M), str(B_), out, kff], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    want = _lines(dump)
    assert open(out).read() == "".join(l + "\n" for l in want)
    _, ents = read_kff(kff)
    assert sorted(f"{km} {idx} {data[0]}" for km, idx, data in ents) == want
    assert run.stdout.splitlines()[-1] == f"nb_kmers {len(dump[0])} nb_buckets {nb_buckets} sum_counts {int(dump[3].astype(np.int64).sum())}"


@pytest.mark.parametrize("mode", ["--facade", "--mixed"])
def test_the_options_are_refused_outside_bulk(tmp_path, mode):
    """no GPU needed: the refusal comes before any device call"""
    for extra in (["--histo", str(tmp_path / "h.tsv")], ["--min-count", "2"], ["--max-count", "9"]):
        run = subprocess.run([_exe(), mode, FASTA, str(K), str(M), str(B_)] + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 2 and "--bulk only" in run.stderr, (run.returncode, run.stderr[-500:])
    assert not os.path.exists(str(tmp_path / "h.tsv"))


def test_bad_option_values_are_refused(tmp_path):
    for extra in (["--min-count", "300"], ["--min-count", "x"], ["--min-count", "5", "--max-count", "2"], ["--histo"]):
        run = subprocess.run([_exe(), "--bulk", FASTA, str(K), str(M), str(B_)] + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 2, (extra, run.returncode, run.stderr[-500:])
