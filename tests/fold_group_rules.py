"""The two fold rules of k_insert_first restated over the oracle's records (DESIGN.md section 4 finding 21); numpy-free, no GPU.

A partition is a list of records in arrival order (a record's position is its lane), each `(bucket, idx0', n, C)` as
tests/insert_clean_reads.py's census keeps them.  `frames()` puts them into the kernel's common frame (fold_frame, fold_core):

    u, m     the string shifted to the frame's end E and the ones over its nucleotides
    ck       [routing id low bits | core]: the bits the lean kernel compares for "same locus"
    sv       (n << 6) | (63 - lane): the order heads are taken in; 0: takes no part
    unsure   takes no part, or reaches below suff_reduc (its windows may miss the core)

`sequential()` is fold_records<NW, true>: one head per wave-wide round, in decreasing sv, at most 16 rounds.
`grouped()` is fold_records_grouped: every lane max-es its sv into the slot `slot(ck)` of 64, reads the slot back and meets the
head it finds there; a head per occupied slot and round.  It hands the partition to the sequential rule where a record is unsure
(containment then need not imply equal ck), where more than 16 heads were taken, or where a lane is open after 16 rounds.
Both return `(per record (folded, lead, off), clean, rounds, heads)`; grouped() adds whether it fell back (its rounds then count
both rules')."""
import insert_clean_reads as R

FOLD_TRIPS = R.FOLD_TRIPS
SLOT_MUL = 0x9E3779B1  # slot(ck): the top six bits of the 32-bit product (fold_slot in brisk_insert.hip)
CORE_BITS = 2 * (R.CORE_NT[1] - R.CORE_NT[0])


def slot(ck):
    return ((ck * SLOT_MUL) & 0xffffffff) >> 26


def frames(recs, rid_bits=4):
    """the kernel's per-lane values for a partition's records; `rid_bits`: the routing-id bits a partition's records differ in"""
    out = []
    for lane, (bucket, i0, n, c) in enumerate(recs):
        end = i0 + n
        ok = n > 0 and end <= R.E and R.E - i0 + R.KB - 1 <= 96
        lo = 2 * (R.E - end) if ok else 0
        m = (((1 << (2 * (R.E - i0 + R.KB - 1))) - 1) ^ ((1 << lo) - 1)) if ok else 0
        u = (c << lo) & m
        core = (u & R.CORE) >> (2 * R.CORE_NT[0])
        out.append({"rid": bucket, "i0": i0, "e": end, "u": u, "m": m, "ck": ((bucket & ((1 << rid_bits) - 1)) << CORE_BITS) | core,
                    "sv": ((n << 6) | (63 - lane)) if ok else 0, "unsure": (not ok) or i0 < R.SUFF})
    return out


def _meet(f, a, test_rid):
    """one lane against head `a`: (contained, makes dirty if it stays open)"""
    same_locus = (f["rid"] == a["rid"]) if test_rid else (f["ck"] == a["ck"])
    inside = same_locus and a["i0"] <= f["i0"] and f["e"] <= a["e"] and (a["u"] & f["m"]) == f["u"]
    return inside, f["ck"] == a["ck"] and f["i0"] < a["e"] and a["i0"] < f["e"]


def sequential(fr):
    assert len(fr) <= 64
    sv = [f["sv"] for f in fr]
    res = [(False, i, 0) for i in range(len(fr))]
    dirty = any(f["unsure"] for f in fr)
    rounds = 0
    for _ in range(FOLD_TRIPS):
        smax = max(sv, default=0)
        if smax == 0:
            break
        rounds += 1
        a = 63 - (smax & 63)
        for i, f in enumerate(fr):
            if sv[i] == 0:
                continue
            inside, meets = _meet(f, fr[a], True)
            if inside:
                sv[i] = 0
                if i != a:
                    res[i] = (True, a, f["i0"] - fr[a]["i0"])
            elif meets:
                dirty = True
    return res, not (dirty or any(sv)), rounds, rounds


def grouped(fr):
    assert len(fr) <= 64
    if any(f["unsure"] for f in fr):
        return sequential(fr) + (True,)
    sv = [f["sv"] for f in fr]
    res = [(False, i, 0) for i in range(len(fr))]
    dirty, rounds, heads = False, 0, 0
    for _ in range(FOLD_TRIPS):
        if not any(sv) or heads > FOLD_TRIPS:
            break
        rounds += 1
        slots = {}
        for i, f in enumerate(fr):
            if sv[i]:
                slots[slot(f["ck"])] = max(slots.get(slot(f["ck"]), 0), sv[i])
        heads += sum(1 for i, f in enumerate(fr) if sv[i] and slots[slot(f["ck"])] == sv[i])
        for i, f in enumerate(fr):
            if sv[i] == 0:
                continue
            a = 63 - (slots[slot(f["ck"])] & 63)
            inside, meets = _meet(f, fr[a], False)
            if inside:
                sv[i] = 0
                if i != a:
                    res[i] = (True, a, f["i0"] - fr[a]["i0"])
            elif meets:
                dirty = True
    if heads > FOLD_TRIPS or any(sv):  # (the rounds spent here are paid as well)
        s = sequential(fr)
        return s[0], s[1], s[2] + rounds, s[3], True
    return res, not dirty, rounds, heads, False


def partitions_of(O, reads, part_shift=4):
    """{partition: records in arrival order} of a read set (flat, offsets); partition = bucket >> part_shift"""
    flat, offs = reads
    raw, o = flat.tobytes(), [int(x) for x in offs]
    h = O.index_new(R.K, R.M, R.B)
    parts = {}
    try:
        for i in range(len(o) - 1):
            c, bucket, n, idx0 = O.records(h, raw[o[i]:o[i + 1]], R.K, R.M, R.B)
            for j in range(len(n)):
                big = sum(int(w) << (64 * t) for t, w in enumerate(c[j]))
                parts.setdefault(int(bucket[j]) >> part_shift, []).append((int(bucket[j]), int(idx0[j]), int(n[j]), big))
    finally:
        O.index_free(h)
    return parts
