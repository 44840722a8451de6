"""CPU: the pair rule of k_insert_first restated over the oracle's records (DESIGN.md section 4 finding 22; tests/insert_pair_rules.py).

  * Pairing changes no (folded, lead, off, clean) result of any record against the per-partition rule: for every neighbouring couple
    whose joint fold stands -- the crafted cases of tests/insert_pair_reads.py, synthetic reads and error-bearing reads at about 12
    records per partition -- each partition's results from the joint fold are the ones of its own fold, and so is its instance count.
  * The instance map over the concatenated list: the multiplicity steps return to zero at the A/B boundary by the kernel's
    `m_first + raw_n < ninst` rule, so every instance's multiplicity is the one its partition's own map gives.
  * The crafted cases are what tests/test_insert_pair.py takes them for: which partitions pair, go alone or are left over."""
import numpy as np
import pytest

import oracle
import fold_group_rules as G
import insert_pair_reads as PR
import insert_pair_rules as RU
from density_reads import dense_reads, _offsets

READS, GENOME = 5000, 6000  # synthetic reads: about 12 records per partition at 2^24 partitions (the error-bearing ones spread over three times as many)


@pytest.fixture(scope="module")
def O():
    oracle.build(ref=False)
    return oracle.Oracle()


@pytest.fixture(scope="module")
def crafted(O):
    return {name: PR.partitions_of(O, PR.pack(PR.case(name))) for name in PR.CASES}


@pytest.fixture(scope="module")
def jobs(O):
    syn = O.synth_reads(GENOME, 0, READS)
    return {"synthetic": PR.partitions_of(O, (np.ascontiguousarray(syn.reshape(-1)), _offsets(np.full(READS, syn.shape[1], np.int64)))),
            "errors": PR.partitions_of(O, dense_reads(READS, PR.K, GENOME, 1, e=0.01))}


def imult(recs, res):
    """the instance map's multiplicities: every record adds 1 over [m_first, m_first + n) of its head's instances (mod 256 left out);
    a step down is written only where it lies inside the list (the kernel's `m_first + raw_n < ninst`)"""
    first, at = [], 0
    for r, (folded, _, _) in zip(recs, res):
        first.append(at)
        at += 0 if folded else r[2]
    diff = [0] * at
    for r, (folded, lead, off) in zip(recs, res):
        m_first = first[lead] + off
        diff[m_first] += 1
        if m_first + r[2] < at:
            diff[m_first + r[2]] -= 1
    return list(np.cumsum(diff)) if at else []


def couples(parts, order):
    for a, b in zip(order, order[1:]):
        if 1 <= len(parts[a]) and 1 <= len(parts[b]) and len(parts[a]) + len(parts[b]) <= RU.MAX_REC:
            yield a, b


def check_couples(parts, order):
    stood = 0
    for a, b in couples(parts, order):
        j = RU.joint(parts[a], parts[b])
        if j is None:
            continue
        stood += 1
        sa, sb = RU.single(parts[a]), RU.single(parts[b])
        assert (j[0], j[1], j[2]) == sa, (a, j[:3], sa)
        assert (j[3], j[4], j[5]) == sb, (b, j[3:], sb)
        # the joint instance map: A's multiplicities, then B's -- nothing carries over the boundary
        na = len(parts[a])
        res = j[0] + [(f, lead + na, off) for f, lead, off in j[3]]
        assert imult(parts[a] + parts[b], res) == imult(parts[a], sa[0]) + imult(parts[b], sb[0]), (a, b)
    return stood


@pytest.mark.parametrize("name", list(PR.CASES))
def test_crafted_cases_are_what_they_are_taken_for(crafted, name):
    parts = crafted[name]
    assert sorted(parts) == [p for p, _ in PR.case(name)]
    assert all(len(parts[p]) == len(reads) for p, reads in PR.case(name))  # one record per read
    out = RU.walk(RU.ascending(parts), parts)
    assert tuple(out[p][0] for p in sorted(parts)) == PR.expect(name), out
    check_couples(parts, sorted(parts))


def test_the_limits_are_exact(crafted):
    inst = lambda name: [RU.single(crafted[name][p])[2] for p in sorted(crafted[name])]
    rec = lambda name: [len(crafted[name][p]) for p in sorted(crafted[name])]
    assert rec("rec-32-32") == [32, 32] and rec("rec-32-33") == [32, 33]
    for f in ("inst", "fold"):
        assert inst(f + "-96-96") == [96, 96] and inst(f + "-1-191") == [1, 191] and inst(f + "-128-64") == [128, 64] and inst(f + "-96-97") == [96, 97, 10]
    assert rec("fold-96-96") > rec("inst-96-96")  # the fold decides the sizes
    assert inst("mixed-big-a")[0] > RU.MAXI and rec("mixed-records")[1] > RU.MAX_REC
    out = RU.walk(RU.ascending(crafted["mixed-overlap"]), crafted["mixed-overlap"])
    a, b = sorted(crafted["mixed-overlap"])
    assert out[a] == ("alone", "not clean", True) and out[b][0] == "alone" and out[b][2] is False  # B by the table path
    out = RU.walk(RU.ascending(crafted["batch-66-shifted"]), crafted["batch-66-shifted"])
    order = sorted(out)
    assert out[order[63]] == ("alone", "batch end", True) and out[order[64]][:2] == ("pair", order[65])  # no pair across lanes 63 | 64


def test_cousin_partitions_hold_the_same_strings(crafted):
    a, b = sorted(crafted["siblings"])
    assert b == a ^ 1
    strings = lambda p: sorted({(bk & 15, i0, n, c) for bk, i0, n, c in crafted["siblings"][p]})
    assert strings(a) == strings(b) and len(strings(a)) == 5  # equal bucket low bits, idx', n and compacted string
    fr = RU.joint_frames(crafted["siblings"][a], crafted["siblings"][b])
    na = len(crafted["siblings"][a])
    assert {f["ck"] & ~(1 << RU.PAIR_BIT) for f in fr[:na]} == {f["ck"] & ~(1 << RU.PAIR_BIT) for f in fr[na:]}  # ... and core
    assert not {f["ck"] for f in fr[:na]} & {f["ck"] for f in fr[na:]}  # the partition bit alone tells them apart
    j = RU.joint(crafted["siblings"][a], crafted["siblings"][b])
    assert j is not None and j[2] == j[5] == RU.single(crafted["siblings"][a])[2]  # nothing folds across: as many instances each
    # without the bit B's records fold into A's heads: the joint list loses B's instances
    fr0 = G.frames(crafted["siblings"][a] + crafted["siblings"][b])
    res0 = G.grouped(fr0)[0]
    assert RU.instances(crafted["siblings"][a] + crafted["siblings"][b], res0) == j[2]


@pytest.mark.parametrize("name", ["synthetic", "errors"])
def test_pairing_changes_no_result_at_working_density(jobs, name):
    parts = jobs[name]
    mean = sum(len(r) for r in parts.values()) / len(parts)
    stood = check_couples(parts, sorted(parts))
    out = RU.walk(sorted(parts), parts)
    t = RU.tally(out)
    print(name, "partitions", len(parts), "records each %.2f" % mean, "joint folds that stand", stood, t)
    assert (8 < mean < 16 if name == "synthetic" else 3 < mean < 16) and stood > 100 and t["pair"] > 0
    assert t["pair"] + t["left"] + sum(t["alone"].values()) == len(parts)
    for p, o in out.items():  # a pair is two clean partitions of at most 64 records and 192 instances together
        if o[0] == "pair" and p < o[1]:
            sa, sb = RU.single(parts[p]), RU.single(parts[o[1]])
            assert sa[1] and sb[1] and sa[2] + sb[2] <= RU.MAXI and len(parts[p]) + len(parts[o[1]]) <= RU.MAX_REC
