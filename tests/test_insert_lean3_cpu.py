"""CPU: the read sets of tests/test_insert_lean3.py are what that test needs them to be (tests/insert_lean3_reads.py; the oracle only).

S3 = partitions of more than 128 distinct k-mers whose counts add up to at most 192, in at most 64 records: k_insert_first must
take them and needs its third instance slot for them.  OVER = more than 192 distinct k-mers or more than 64 records: it must
leave them over.  AMBIG = at most 192 distinct k-mers but more instances before the containment fold: either.  The GPU test
asserts OVER <= left <= OVER + AMBIG, which a kernel that refused the three-slot partitions cannot meet only if AMBIG < S3."""
import pytest

import oracle
import insert_lean3_reads as R


@pytest.fixture(scope="module")
def O():
    oracle.build(ref=False)
    return oracle.Oracle()


@pytest.fixture(scope="module")
def censuses(O):
    return {"one": R.census(O, R.set_one()), "two": R.census(O, R.set_two())}


@pytest.mark.parametrize("which", ["one", "two"])
def test_the_sets_cannot_pass_without_the_third_slot(censuses, which):
    c = censuses[which]
    assert all(c["at"][n] >= 20 for n in R.CLASSES), c  # every boundary class is there
    assert c["S3"] >= 20 and c["OVER"] >= 5 and c["AMBIG"] < c["S3"], c
    assert c["many_records"] >= 5 and c["OVER"] >= c["at"][193] + c["many_records"], c
    assert c["partitions"] > 20 * (c["S3"] + c["OVER"]), c  # ordinary partitions around them


def test_set_one_covers_every_kmer_of_its_loci_once(censuses):
    c = censuses["one"]
    assert c["exact"] == c["at"] and c["AMBIG"] == 0 and c["folding"] == 0, c
    assert c["S3"] == c["at"][129] + c["at"][191] + c["at"][192], c


def test_set_two_has_contained_records_on_three_slot_partitions(censuses):
    c = censuses["two"]
    assert c["folding"] >= 40 and c["AMBIG"] >= 5, c  # the fold has records to close; some partitions hang on what it closes
    assert c["exact"][129] == 0 and c["at"][129] >= 20, c  # every 129-k-mer locus is covered more than once somewhere, within 192 in all


def test_the_hot_locus_is_a_192_kmer_partition_of_set_one(O):
    reads, copy = R.hot_locus()
    c = R.census(O, R._pack(reads))
    assert c["partitions"] == 1 and c["exact"][192] == 1 and copy in reads, c
