"""The pair rule of k_insert_first restated over the oracle's records (DESIGN.md section 4 finding 22); numpy-free, no GPU.  Built on
tests/fold_group_rules.py: a partition is a list of records in arrival order, each `(bucket, idx0', n, C)`.

A wave walks its batch of 64 touched partitions.  Where it requests the next partition's records it looks at the next two
descriptors, A and B, and loads B's records behind A's -- lanes [nA, nA + nB) -- when both are first-fill candidates (a fresh index:
every partition; 1 <= n_rec), nA + nB <= 64 and B lies inside the batch.  The two then run one grouped fold, their `ck` told apart by
a partition bit.  What makes the joint grouped fold fail (an unsure record, more than 16 heads in all, a lane open after 16 rounds)
un-pairs: A goes alone from the top.  After the fold the pair goes on only if both partitions are clean -- no lane of theirs is
dirty -- and their instances together are at most 192; otherwise A goes alone from the joint fold's results for its lanes, and B
heads the next candidate pair.

`walk(order, parts)` gives every partition's outcome:

    ("pair", partner, clean=True)       taken with its neighbour, table-free
    ("alone", reason, clean)            taken alone; reason: why it did not pair as A (see REASONS)
    ("left", reason)                    left over to k_insert_fast_listed: more than 64 records, or more than 192 instances

The order of the touched list is the device's: ascending inside a block of 8192 partitions (k_touched), the blocks in the order
their atomics land.  `ascending(parts)` is that order where all partitions lie in one block; a job over many blocks is walked in the
order the library reports (BriskHip.debug_touched)."""
import fold_group_rules as G

MAXI = 192          # instances k_insert_first takes (three slots per lane)
MAX_REC = 64        # records: one per lane
BATCH = 64          # partitions a wave takes at once (WI_BATCH)
TOUCHED_BLOCK = 8192
PAIR_BIT = 18       # ck's partition bit at the flagship geometry: above [routing id low bits : 4 | core : 14]
REASONS = ("batch end", "records", "fold", "not clean", "instances", "partner left")


def joint_frames(recs_a, recs_b, rid_bits=4):
    """the kernel's per-lane values for A's records and B's behind them; B's ck carries the partition bit"""
    fr = G.frames(list(recs_a) + list(recs_b), rid_bits)
    bit = 1 << max(PAIR_BIT, rid_bits + G.CORE_BITS)
    for f in fr[len(recs_a):]:
        assert f["ck"] < bit
        f["ck"] |= bit
    return fr


def grouped_lanes(fr):
    """fold_records_grouped with the lanes it found dirty: (per record (folded, lead, off), set of dirty lanes, rounds, heads), or None
    where the kernel's returns false (an unsure record, more than 16 heads, a lane open after the last round)"""
    assert len(fr) <= MAX_REC
    if any(f["unsure"] for f in fr):
        return None
    sv = [f["sv"] for f in fr]
    res = [(False, i, 0) for i in range(len(fr))]
    dirty, rounds, heads = set(), 0, 0
    for _ in range(G.FOLD_TRIPS):
        if not any(sv) or heads > G.FOLD_TRIPS:
            break
        rounds += 1
        slots = {}
        for i, f in enumerate(fr):
            if sv[i]:
                slots[G.slot(f["ck"])] = max(slots.get(G.slot(f["ck"]), 0), sv[i])
        heads += sum(1 for i, f in enumerate(fr) if sv[i] and slots[G.slot(f["ck"])] == sv[i])
        for i, f in enumerate(fr):
            if sv[i] == 0:
                continue
            a = 63 - (slots[G.slot(f["ck"])] & 63)
            inside, meets = G._meet(f, fr[a], False)
            if inside:
                sv[i] = 0
                if i != a:
                    res[i] = (True, a, f["i0"] - fr[a]["i0"])
            elif meets:
                dirty.add(i)
    if heads > G.FOLD_TRIPS or any(sv):
        return None
    return res, dirty, rounds, heads


def instances(recs, res):
    """k-mer instances after the fold: the n of the records that did not fold"""
    return sum(r[2] for r, (folded, _, _) in zip(recs, res) if not folded)


def single(recs, rid_bits=4):
    """the per-partition rule (today's single route): (per record (folded, lead, off), clean, instances)"""
    res, clean = G.grouped(G.frames(recs, rid_bits))[:2]
    return res, clean, instances(recs, res)


def joint(recs_a, recs_b, rid_bits=4):
    """the joint fold of a candidate pair: None where it does not stand, else (res_a, clean_a, ninst_a, res_b, clean_b, ninst_b) with
    B's leads counted from B's first lane, so that each triple is comparable with single()'s"""
    g = grouped_lanes(joint_frames(recs_a, recs_b, rid_bits))
    if g is None:
        return None
    res, dirty = g[:2]
    na = len(recs_a)
    assert all(lead < na for _, lead, _ in res[:na]) and all(lead >= na for _, lead, _ in res[na:]), "a record met a head of the other partition"
    res_a, res_b = res[:na], [(f, lead - na, off) for f, lead, off in res[na:]]
    return (res_a, not any(i < na for i in dirty), instances(recs_a, res_a), res_b, not any(i >= na for i in dirty), instances(recs_b, res_b))


def ascending(parts):
    order = sorted(parts)
    assert order and order[0] // TOUCHED_BLOCK == order[-1] // TOUCHED_BLOCK, "more than one block of the touched list: its order is the device's"
    return order


def walk(order, parts, rid_bits=4, need_clean=True, maxi=MAXI):
    """{partition: outcome} of a first batch into a fresh index whose touched list is `order`.  need_clean=False: the rule without
    its clean condition (what a table path for pairs would add; the census prints it, the kernel does not do it)."""
    out = {}
    for t0 in range(0, len(order), BATCH):
        t_end, t = min(t0 + BATCH, len(order)), t0
        while t < t_end:
            pa = order[t]
            a = parts[pa]
            if len(a) > MAX_REC:
                out[pa] = ("left", "records")
                t += 1
                continue
            reason, known = None, None
            if t + 1 >= t_end:
                reason = "batch end"
            else:
                pb = order[t + 1]
                b = parts[pb]
                if len(b) > MAX_REC:
                    reason = "partner left"
                elif len(a) + len(b) > MAX_REC:
                    reason = "records"
                else:
                    j = joint(a, b, rid_bits)
                    if j is None:
                        reason = "fold"
                    else:
                        res_a, clean_a, ni_a, res_b, clean_b, ni_b = j
                        known = (clean_a, ni_a)  # (A goes on from the joint fold's results)
                        if need_clean and not (clean_a and clean_b):
                            reason = "not clean"
                        elif ni_a + ni_b > maxi:
                            reason = "instances"
                        else:
                            out[pa] = ("pair", pb, clean_a)
                            out[pb] = ("pair", pa, clean_b)
                            t += 2
                            continue
            clean, ninst = known if known is not None else single(a, rid_bits)[1:]
            out[pa] = ("left", "instances") if ninst > maxi else ("alone", reason, clean)
            t += 1
    return out


def tally(outcome):
    """counts of a walk: partitions in pairs, alone by reason, left over"""
    n = {"pair": 0, "left": 0, "alone": {r: 0 for r in REASONS}}
    for o in outcome.values():
        if o[0] == "alone":
            n["alone"][o[1]] += 1
        else:
            n[o[0]] += 1
    return n


def passes(outcome, parts, rid_bits=4):
    """instance passes of 64 (single scheme, pair scheme) summed over the partitions k_insert_first takes"""
    ninst = {p: single(parts[p], rid_bits)[2] for p, o in outcome.items() if o[0] != "left"}
    one = sum((n + 63) // 64 for n in ninst.values())
    two = sum((ninst[p] + 63) // 64 for p, o in outcome.items() if o[0] == "alone")
    two += sum((ninst[p] + ninst[o[1]] + 63) // 64 for p, o in outcome.items() if o[0] == "pair" and p < o[1])
    return one, two, len(ninst)
