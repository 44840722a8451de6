"""No device: the intake rule in numpy (brisk_amd.fragments_from_reads) against the oracle's restatement of clean_dna
(oracle.fasta_sequences), its quality cut, and the C-ABI's new symbols and struct sizes."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from intake_reference import crafted_case, fragment_strings, most_fragments_in_a_word, expected_outputs

import brisk_amd
from brisk_amd import hipapi

K = 31
# characters that Python's str.splitlines / str.strip take for line breaks or blanks: oracle.fasta_sequences would join a record
# across them, where clean_dna (which sees the record after getline) cuts at them like at any other non-base.  They are non-bases on
# both sides; the oracle gets '-' in their place so that its own line handling stays out of the comparison.  Positions do not move.
_BREAKS = "".join(chr(c) for c in range(256) if chr(c).isspace() or len(("a" + chr(c) + "b").splitlines()) > 1)


def body_of(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return "".join(line.strip() for line in f.read().splitlines() if not line.startswith(">"))


def random_bodies(n, seed):
    rng = random.Random(seed)
    alphabet = "ACGTacgtNnRY-\r" + "".join(chr(c) for c in (0x80, 0x85, 0xa0, 0xc3, 0xff))
    out = []
    for i in range(n):
        p_bad = rng.choice((0.002, 0.02, 0.1, 0.5))
        out.append("".join(rng.choice(alphabet[8:]) if rng.random() < p_bad else rng.choice(alphabet[:8]) for _ in range(rng.randint(0, 400))))
    return out


def independent_fragments(bodies, k):
    """(read, start, len) by regular expression: a third statement of the rule, for the table's fields"""
    rows = []
    for r, b in enumerate(bodies):
        rows += [(r, m.start(), m.end() - m.start()) for m in re.finditer("[ACGTacgt]+", b) if m.end() - m.start() >= k]
    return rows


def test_no_quality_cut_is_the_oracles_clean_dna():
    bodies = [body_of("test.fa"), body_of("debug_test.fa")] + random_bodies(300, 31)
    frags, st = brisk_amd.fragments_from_reads(bodies, None, K)
    got = [s.decode("latin-1").upper() for s in fragment_strings(bodies, frags)]
    want = []
    n_dropped = 0
    for b in bodies:
        seqs = [s for s in oracle.fasta_sequences(">\n" + b.translate({ord(c): "-" for c in _BREAKS})) if s]
        n_dropped += sum(len(s) < K for s in seqs)
        want += [s for s in seqs if len(s) >= K]
    assert got == want
    assert [(int(f["read"]), int(f["start"]), int(f["len"])) for f in frags] == independent_fragments(bodies, K)
    assert n_dropped > 100 and len(want) > 100, "the cases hold kept and dropped runs"
    assert st["n_bases_in"] == sum(len(b) for b in bodies) == st["n_nts"] + st["n_cut_base"] + st["n_cut_qual"] + st["n_short"]
    assert st["n_fragments"] == len(want) and st["n_nts"] == sum(len(s) for s in want) and st["n_cut_qual"] == 0 and st["n_short"] > 0
    assert st["n_reads"] == len(bodies) and st["n_reads_kept"] == len({int(f["read"]) for f in frags}) < len(bodies)


@pytest.mark.parametrize("qual_base", [33, 64])
def test_quality_threshold(qual_base):
    thr = qual_base + 20
    seq = b"ACGTACGTNACGTAC"
    qual = bytes([thr] * 4 + [thr - 1] + [thr + 1] * 3 + [0] + [thr] * 2 + [thr - 1] + [255, thr, thr])
    frags, st = brisk_amd.fragments_from_reads([seq], [qual], 3, brisk_amd.intake_rule(min_qual=20, qual_base=qual_base))
    # exactly at the threshold: kept; one below: cut; the N's low quality is a base cut, not a quality cut
    assert [(int(f["start"]), int(f["len"])) for f in frags] == [(0, 4), (5, 3), (12, 3)]
    assert st == {"n_reads": 1, "n_reads_kept": 1, "n_fragments": 3, "n_bases_in": 15, "n_nts": 10, "n_cut_base": 1, "n_cut_qual": 2, "n_short": 2}
    # min_qual 0: the qualities are ignored, and may be absent
    for quals in ([qual], None):
        frags, st = brisk_amd.fragments_from_reads([seq], quals, 3, brisk_amd.intake_rule())
        assert [(int(f["start"]), int(f["len"])) for f in frags] == [(0, 8), (9, 6)] and st["n_cut_qual"] == 0
    if qual_base == 33:  # qual_base 0 means 33
        assert brisk_amd.fragments_from_reads([seq], [qual], 3, brisk_amd.intake_rule(min_qual=20, qual_base=0))[1] == \
            brisk_amd.fragments_from_reads([seq], [qual], 3, brisk_amd.intake_rule(min_qual=20))[1]


def test_the_definition_refuses_what_the_library_refuses():
    for rule in (brisk_amd.intake_rule(min_qual=94), brisk_amd.intake_rule(qual_base=50)):
        with pytest.raises(ValueError):
            brisk_amd.fragments_from_reads([b"ACGT"], [b"IIII"], 3, rule)
    with pytest.raises(ValueError):
        brisk_amd.fragments_from_reads([b"ACGT"], None, 3, brisk_amd.intake_rule(min_qual=1))
    with pytest.raises(ValueError):
        brisk_amd.fragments_from_reads([b"ACGT"], [b"III"], 3, brisk_amd.intake_rule(min_qual=1))


@pytest.mark.parametrize("L", [5, 31])
def test_crafted_case_holds_what_the_gpu_test_needs(L):
    for variant in (0, 1):
        reads, facts = crafted_case(L, variant)
        assert facts["run_align"] == {(n, a) for n in range(1, 41) for a in range(16)}
        assert facts["boundary_align"] == set(range(16)) and facts["valid_boundary"] >= 16
        assert facts["total"] % 16 != 0 and facts["total"] > 2 * hipapi.INTAKE_BLOCK
        assert (facts["first_valid"], facts["last_valid"]) == ((True, False) if variant == 0 else (False, True))
        lens = [len(r) for r in reads]
        assert lens[0] == 0 and lens[-1] == 0 and 1 in lens and any(a == 0 and b == 0 for a, b in zip(lens, lens[1:]))
        frags, st = brisk_amd.fragments_from_reads(reads, None, L)
        assert L in frags["len"] and st["n_short"] > 0 and st["n_fragments"] > 200
        words, starts = expected_outputs(reads, frags)
        assert len(words) == (st["n_nts"] + 15) // 16 + 2 and int(starts[-1]) == st["n_nts"]
        if L == 5:
            assert most_fragments_in_a_word(starts) >= 4


def test_library_exports_and_struct_sizes():
    L = hipapi.load()
    for s in ("brisk_hip_intake_ascii", "brisk_hip_intake_reads", "brisk_hip_insert_raw_reads"):
        assert hasattr(L, s) and s in hipapi.SYMBOLS
    assert L.brisk_hip_abi_version() == 4
    assert (C.sizeof(hipapi._IntakeRule), C.sizeof(hipapi._Fragment), C.sizeof(hipapi._IntakeStats)) == (16, 16, 64)
    assert hipapi.FRAGMENT_DTYPE.itemsize == 16 and len(hipapi.INTAKE_STATS_FIELDS) == 8
    header = open(os.path.join(hipapi.ROOT, "include", "brisk_hip.h")).read()
    assert "#define BRISK_HIP_INTAKE_BLOCK %d" % hipapi.INTAKE_BLOCK in header


# ---- the host FASTQ reader (brisk_amd/include/brisk_fastq.hpp) through tests/cpp/fastq_dump.cpp
@pytest.fixture(scope="module")
def dumper(tmp_path_factory):
    import subprocess
    exe = str(tmp_path_factory.mktemp("bin") / "fastq_dump")
    subprocess.check_call(["g++", "-std=gnu++17", "-O2", "-pthread", "-I" + os.path.join(os.path.dirname(brisk_amd.__file__), "include"),
                           os.path.join(hipapi.ROOT, "tests", "cpp", "fastq_dump.cpp"), "-lz", "-o", exe])
    return exe


def dump(dumper, path, batch):
    import subprocess
    out = subprocess.run([dumper, str(path), str(batch)], capture_output=True, text=True, timeout=120)
    lines = out.stdout.split("\n")[:-1]
    records = [tuple(l.split("\t")) for l in lines if not l.startswith("#")]
    batches = [int(l.split()[1]) for l in lines if l.startswith("#batch")]
    return out.returncode, records, batches, out.stderr


def fastq_records(n, seed):
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        m = 0 if i in (3, n - 1) else rng.randint(1, 200)  # an empty sequence line, in the middle and as the last record
        recs.append(("".join(rng.choice("ACGTN") for _ in range(m)), "".join(chr(rng.randint(33, 126)) for _ in range(m))))
    return recs


def fastq_text(recs, eol="\n", last_eol=True):
    lines = []
    for i, (s, q) in enumerate(recs):
        lines += ["@read%d some text" % i, s, "+" if i % 2 else "+read%d" % i, q]
    return eol.join(lines) + (eol if last_eol else "")


def test_fastq_reader(dumper, tmp_path):
    import gzip
    recs = fastq_records(3000, 8)
    plain = tmp_path / "r.fq"
    plain.write_text(fastq_text(recs))
    want = [(s, q) for s, q in recs]
    rc, got, batches, err = dump(dumper, plain, 1000)
    assert rc == 0 and got == want and len(batches) > 100 and sum(batches) == len(recs), err
    for batch in (1, 1 << 20):  # one record a batch; everything in one batch
        rc, got, batches, err = dump(dumper, plain, batch)
        assert rc == 0 and got == want, err
        # (a record without bases does not fill a batch of one byte: it rides with the record after it, or ends the file)
        assert (len(batches) == len(recs) - 1 and set(batches) == {1, 2}) if batch == 1 else batches == [len(recs)]
    gz = tmp_path / "r.fq.gz"
    with gzip.open(gz, "wt") as f:
        f.write(fastq_text(recs))
    crlf = tmp_path / "crlf.fq"
    crlf.write_bytes(fastq_text(recs, eol="\r\n").encode())
    open_end = tmp_path / "open.fq"
    open_end.write_text(fastq_text(recs[:-1], last_eol=False))
    open_end_crlf = tmp_path / "open_crlf.fq"
    open_end_crlf.write_bytes(fastq_text(recs[:-1], eol="\r\n", last_eol=False).encode())
    for path, n in ((gz, len(recs)), (crlf, len(recs)), (open_end, len(recs) - 1), (open_end_crlf, len(recs) - 1)):
        rc, got, batches, err = dump(dumper, path, 1000)
        assert rc == 0 and got == want[:n], (path, err)
    empty = tmp_path / "empty.fq"
    empty.write_text("")
    assert dump(dumper, empty, 1000)[:3] == (0, [], [])


def test_fastq_reader_refuses_malformed_records(dumper, tmp_path):
    recs = fastq_records(40, 9)
    lines = fastq_text(recs).split("\n")
    bad_qual, no_plus, no_at, cut_short = list(lines), list(lines), list(lines), lines[:4 * 20 + 2]
    bad_qual[4 * 10 + 3] += "I"           # record 11: a quality line one character too long
    no_plus[4 * 6 + 2] = "ACGT"           # record 7: a second sequence line where the '+' belongs
    no_at[4 * 24] = ">read24"             # record 25: a FASTA header
    for name, text, record in (("qual", bad_qual, 11), ("plus", no_plus, 7), ("at", no_at, 25), ("cut", cut_short, 21)):
        path = tmp_path / (name + ".fq")
        path.write_text("\n".join(text) + ("" if name == "cut" else "\n"))
        rc, got, batches, err = dump(dumper, path, 300)
        assert rc == 1 and ("FASTQ record %d:" % record) in err, (name, err)
