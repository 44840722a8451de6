"""The sharded per-k-mer get on ONE device, shared by tests/test_sharded_kmers.py, its workers and
tests/test_sharded_kmers_cpu.py.  Nothing here is a test.  Inputs and the N-owner job come from tests/sharded_cases.py and
tests/sharded_job.py; the expected slots from tests/test_kmer_query.py (expected_all over the oracle's index).

round_trip() plays asker and owners through the C-ABI -- scan_kmers, route_tagged, record_kmers, answer_records on each owner,
place_answers piece by piece -- and asserts on the way, in numpy:

  routing        range and conservation of (tag, record) pairs (sharded_job.check_routed)
  offsets        record_kmers' table is the host prefix sum of the records' k-mer counts, on the asker and on every owner
  answers        the owners' answer counts add up to n_slots, n_slots is kmer_slots of the reads, every answer entry is written
  slots          the slot array is filled with 0xFFFF first (no slot value looks like that) and none remains: with as many answers
                 as slots, each stored to one slot in range (place_answers returned OK), every slot was written exactly once

facts() says, from the oracle alone, what a case exercises (tests/test_sharded_kmers_cpu.py holds every case to it)."""
import numpy as np

import oracle
import sharded_cases as C
import sharded_job as S

KMER_GEOMETRIES = [(63, 21, 14), (31, 11, 4), (31, 15, 14), (47, 15, 10)]  # (31, 11, 4): hash and class bits in the routing id; (47, 15, 10): the generic probe body
KMER_OWNER_COUNTS = [2, 3, 8]
# equal ranges; cut points balanced on the job's histogram; cut points that leave owners empty: with 8 owners the first, a middle and
# the last one at once, with 3 each of the three in turn (with 2 an empty owner would leave one owner with everything)
CUT_SCHEMES = [("equal", n) for n in KMER_OWNER_COUNTS] + [("balanced", n) for n in KMER_OWNER_COUNTS] + [("empty", 8), ("empty first", 3), ("empty middle", 3), ("empty last", 3)]
SOLID_MINS = (0, 2, 300)
FILL = 0xFFFF


PROFILE_GEOMETRIES = [(63, 21, 14), (31, 15, 14)]  # 150 nt reads: 88 and 120 slots, segments under BRISK_PROFILE_SEG=64
RANK_BATCH_READS = 256


def wrap_case(k):
    """(reads, queries, the hot read): one read of k + 20 nt 256 times -- stored count 0 in a wrapping index, 255 in a saturating
    one -- among 300 base reads; the queries start with the hot read"""
    import random
    rng = random.Random(256 + k)
    hot = "".join(rng.choice("ACGT") for _ in range(k + 20))
    return [hot] * 256 + C.saturate_reads(), [hot] + C.base_queries()[:60] + C.base_queries()[-40:], hot


def rank_queries(rank):
    """what rank `rank` of the four-rank job asks for: some of its own reads, then reads that are not in the index; 256 reads a
    batch make two batches on ranks 0, 1 and 3 and one on rank 2, which idles in the second"""
    import random
    mine = [s for i in range(len(C.RANK_SHARES)) for s in C.rank_reads(i, rank)]
    rng = random.Random(900 + rank)
    absent = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(40 + rank)]
    return [(s.decode() if isinstance(s, bytes) else s).upper() for s in mine[:(300, 300, 100, 230)[rank]]] + absent


def scheme_id(s):
    return "%s-%d" % (s[0].replace(" ", "-"), s[1])


def cuts_of(scheme, n_owners, reads, k, m, b, part_bits=0):
    """the cut points of a scheme, from the oracle's records of the job alone (None: equal ranges)"""
    if scheme == "equal":
        return None
    part, n, lay = S.oracle_partitions(reads, k, m, b, part_bits)
    pb = lay["part_bits"]
    if scheme == "balanced":
        import torch
        from brisk_amd import exchange as X
        uniq, words = S.sparse_hist(part, n)
        if pb <= 24:
            hist = np.zeros(1 << pb, np.int64)
            hist[uniq] = words
            return X.balanced_cuts(torch.from_numpy(hist), pb, n_owners)
        blocks = np.zeros(1 << 14, np.int64)  # (coarse_sums of a histogram too large to build here)
        np.add.at(blocks, uniq >> (pb - 14), words >> 32)
        return X.cuts_from_coarse(torch.from_numpy(blocks), pb, n_owners)
    empty = {"empty": (0, n_owners // 2, n_owners - 1), "empty first": (0,), "empty middle": (n_owners // 2,), "empty last": (n_owners - 1,)}[scheme]
    full = [o for o in range(n_owners) if o not in empty]
    inner = S.cuts_at_records(part, pb, len(full))  # cut points on partitions that hold records, for the owners that hold some
    cuts, at = [0], 0
    for o in range(n_owners):  # an owner that holds records ends where its share of them ends, an empty one where it starts
        at += o in full
        cuts.append(inner[at] if o in full else cuts[-1])
    assert cuts[0] == 0 and cuts[-1] == 1 << pb and cuts == sorted(cuts), cuts
    assert all((cuts[o + 1] == cuts[o]) == (o in empty) for o in range(n_owners)), (scheme, cuts)
    return cuts


# ---- the oracle's side -------------------------------------------------------------------------------------------------------------
def expected(reads, queries, k, m, b):
    """(slots, alternatives, slot bases) of `queries` against the oracle's index of `reads` (test_kmer_query.expected_all), once"""
    def make():
        from test_kmer_query import expected_all, oracle_index
        O = S.the_oracle()
        h = oracle_index(O, reads, k, m, b)
        out = expected_all(O, h, queries, k, m)
        O.index_free(h)
        return out
    return S._once(("kmers expected", k, m, b, hash(tuple(reads)), hash(tuple(queries))), make)


def resolved(want, alts, got):
    """the oracle's slots with, for every vector that is its own reverse complement, the orientation the device took (both are the
    oracle's values; assert_slots accepts either): what the reductions over the device's slots are held to"""
    want = want.copy()
    for s, e, v in alts:
        if np.array_equal(got[s:e], v):
            want[s:e] = v
    return want


def expected_profile(want, base, solid_min):
    import brisk_amd
    return brisk_amd.profile_from_slots((want & 0xff).astype(np.uint8), (want & 0x100) != 0, base, solid_min)


def orientations(O, read, k, m):
    """(forward, reverse): how many of the enumerator's vectors over `read` are the read's own k-mers (ascending slots) and how many
    their reverse complements (descending slots) -- expected_slots' `fwd` and `rev`, vectors that are both left out"""
    from test_kmer_query import _codes, _window_words
    codes = _codes(read)
    if len(codes) < k:
        return 0, 0
    f_lo, f_hi = _window_words(codes, k)
    r_lo, r_hi = _window_words((codes ^ 2)[::-1].copy(), k)
    r_lo, r_hi = r_lo[::-1], r_hi[::-1]
    _, skm_n, lo, hi, _, _ = O.enumerate(read, k, m)
    p = t = nf = nr = 0
    for n in skm_n:
        n = int(n)
        fwd = np.array_equal(lo[t:t + n], f_lo[p:p + n]) and np.array_equal(hi[t:t + n], f_hi[p:p + n])
        rev = np.array_equal(lo[t:t + n], r_lo[p:p + n][::-1]) and np.array_equal(hi[t:t + n], r_hi[p:p + n][::-1])
        nf += fwd and not rev
        nr += rev and not fwd
        p += n
        t += n
    return nf, nr


def facts(reads, queries, k, m, b, part_bits=0, cls_env=-1):
    """What the queries' records look like, from the oracle alone: per record piece its partition, whether any of its k-mers is in the
    oracle's index of `reads` and whether none is; and the vectors' orientations (forward, reverse)."""
    def make():
        from test_kmer_query import oracle_index
        O = S.the_oracle()
        lay = S.layout_of(k, m, b, part_bits, cls_env)
        pieces, kmers = S.oracle_pieces(queries, k, m, b, lay)
        h = oracle_index(O, reads, k, m, b)
        present, nf, nr = [], 0, 0
        for q in queries:
            q = q.decode() if isinstance(q, bytes) else q
            if len(q) < k:
                continue
            _, _, lo, hi, idx, _ = O.enumerate(q, k, m)
            assert len(lo) == len(q) - k + 1
            present += [O.index_get(h, int(a), int(c), int(i)) >= 0 for a, c, i in zip(lo, hi, idx)]
            f, r = orientations(O, q, k, m)
            nf, nr = nf + f, nr + r
        O.index_free(h)
        assert len(present) == len(kmers) == int(pieces[:, 1].sum())
        present = np.array(present, bool)
        ends = np.cumsum(pieces[:, 1])
        hits = np.add.reduceat(present.astype(np.int64), ends - pieces[:, 1]) if len(pieces) else np.zeros(0, np.int64)
        part = pieces[:, 0] >> (2 * b + lay["ext_bits"] - lay["part_bits"])
        return dict(part=part, any_present=hits > 0, all_absent=hits == 0, forward=nf, reverse=nr, part_bits=lay["part_bits"])
    return S._once(("kmers facts", k, m, b, part_bits, cls_env, hash(tuple(reads)), hash(tuple(queries))), make)


def assert_not_vacuous(f, cuts, what):
    """at least two owners own records with present k-mers, both vector orientations occur, some records hold absent k-mers only"""
    owners = set(S.owner_of(f["part"][f["any_present"]], cuts).tolist())
    assert len(owners) >= 2, (what, "owners with present k-mers", sorted(owners))
    assert f["forward"] > 0 and f["reverse"] > 0, (what, "orientations", f["forward"], f["reverse"])
    assert f["all_absent"].any(), (what, "no record of absent k-mers only")


# ---- the device's side -------------------------------------------------------------------------------------------------------------
def host_offsets(rec):
    return np.concatenate([[0], np.cumsum(S.instances(rec))]).astype(np.uint64)


class Trip:
    """what round_trip leaves on the device and what it learnt: .slots (uint16, host), .n_slots, .nq, .counts, and the tensors
    d_packed, d_starts, d_out, d_tags_out, d_anchors, d_offs (the asker's table over all routed records), d_answers, d_slots"""


def round_trip(job, queries):
    """The per-k-mer get of `queries` over the open owners of a Job (asker: owner 0's handle), the asserts of the module's docstring
    on the way.  Returns a Trip."""
    import brisk_amd
    import torch
    owners, cuts = job.owners, job.cuts
    ix0 = owners[0]
    W, lay, k = ix0.record_words, ix0.layout, ix0.k
    t = Trip()
    t.d_packed, t.d_starts = d_packed, d_starts = S.to_device(ix0, queries)
    n = len(queries)
    bound = ix0.scan_bound(d_starts.data_ptr(), n)
    d_rec = torch.zeros(max(bound, 1) * W, dtype=torch.int64, device="cuda")
    t.d_out = d_out = torch.zeros_like(d_rec)
    d_tags = torch.zeros(max(bound, 1), dtype=torch.int32, device="cuda")
    t.d_tags_out = d_tags_out = torch.zeros_like(d_tags)
    t.d_anchors = d_anchors = torch.zeros(max(bound, 1), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t.nq, t.n_slots = nq, n_slots = ix0.scan_kmers(d_packed.data_ptr(), d_starts.data_ptr(), n, d_rec.data_ptr(), d_tags.data_ptr(), d_anchors.data_ptr(), bound)
    _, offs_reads = oracle.pack_reads(queries)
    assert n_slots == int(brisk_amd.kmer_slots(offs_reads, k)[-1]), ("n_slots", n_slots)
    t.counts = counts = [int(c) for c in ix0.route_tagged(d_rec.data_ptr(), d_tags.data_ptr(), nq, d_out.data_ptr(), d_tags_out.data_ptr())]
    assert sum(counts) == nq
    tags, tags_out = d_tags[:nq].cpu().numpy().view(np.uint32), d_tags_out[:nq].cpu().numpy().view(np.uint32)
    assert np.array_equal(tags, np.arange(nq, dtype=np.uint32)), "scan_kmers: d_tags[i] indexes the anchor of record i"
    rec_out = S.host_rows(d_out, nq, W)
    S.check_routed(S.host_rows(d_rec, nq, W), rec_out, counts, cuts, lay, ix0.b, tags, tags_out)
    t.d_offs = d_offs = torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix0.record_kmers(d_out.data_ptr() if nq else 0, nq, d_offs.data_ptr())
    offs = d_offs.cpu().numpy().view(np.uint64)
    assert np.array_equal(offs, host_offsets(rec_out)), "record_kmers on the asker"
    assert int(offs[-1]) == n_slots, ("the records' k-mers are the batch's slots", int(offs[-1]), n_slots)
    t.d_answers = d_answers = torch.full((max(n_slots, 1),), 0x7777, dtype=torch.int16, device="cuda")
    t.d_slots = d_slots = torch.full((max(n_slots, 1),), -1, dtype=torch.int16, device="cuda")  # 0xFFFF
    torch.cuda.synchronize()
    at, owed = 0, []
    for o, ix in enumerate(owners):
        c = counts[o]
        if cuts[o + 1] == cuts[o]:
            assert c == 0, "an owner without partitions received records"
        rec_ptr = d_out.data_ptr() + at * W * 8
        ans_ptr = d_answers.data_ptr() + int(offs[at]) * 2
        d_own = torch.full((c + 1,), -1, dtype=torch.int64, device="cuda")  # the owner's table, from the records it received
        torch.cuda.synchronize()
        ix.record_kmers(rec_ptr if c else 0, c, d_own.data_ptr())
        own = d_own.cpu().numpy().view(np.uint64)
        assert np.array_equal(own, offs[at:at + c + 1] - offs[at]), ("record_kmers on owner", o)
        ix.answer_records(rec_ptr if c else 0, c, d_own.data_ptr(), ans_ptr)
        owed.append(int(own[-1]))
        # the asker places this owner's piece: its records, their tags, the piece's table, the answers that came back for it
        ix0.place_answers(rec_ptr if c else 0, d_tags_out.data_ptr() + at * 4, d_anchors.data_ptr(), c, d_own.data_ptr(), ans_ptr, d_slots.data_ptr(), n_slots)
        at += c
    torch.cuda.synchronize()
    assert sum(owed) == n_slots, ("answer counts per owner", owed, n_slots)
    answers = d_answers[:n_slots].cpu().numpy().view(np.uint16)
    assert not (answers == 0x7777).any(), "answer_records left entries unwritten"
    t.slots = slots = d_slots[:n_slots].cpu().numpy().view(np.uint16)
    assert not (slots == FILL).any(), ("slots never written", int((slots == FILL).sum()))
    assert np.array_equal(np.sort(slots), np.sort(answers)), "the slots are not the answers, moved"
    return t


def profile_slots(ix, d_slots, d_starts, n_reads, solid_min):
    """(records on the host, the same on the device)"""
    import brisk_amd
    import torch
    d_out = torch.full((max(n_reads, 1) * 32,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ix.profile_slots(d_slots.data_ptr(), d_starts.data_ptr(), n_reads, d_out.data_ptr(), solid_min)
    return d_out.cpu().numpy().view(brisk_amd.READ_PROFILE_DTYPE)[:n_reads], d_out


def assert_same_records(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for f in want.dtype.names:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (what, f, int(bad[0]), got[bad[0]], want[bad[0]], len(bad))


def check_profiles(ix, t, want, base, n_reads, what):
    """profile_slots over the placed slots against profile_from_slots of the oracle's slots at every solid_min; the solid_run and
    median rules over the device's records against intervals_from_profile of the oracle's"""
    import brisk_amd
    import torch
    for s in SOLID_MINS:
        got, d_prof = profile_slots(ix, t.d_slots, t.d_starts, n_reads, s)
        prof = expected_profile(want, base, s)
        assert_same_records(got, prof, (what, "profile_slots", s))
        if s == 2:
            assert (prof["n_solid"] > 0).any() and (prof["n_solid"] == 0).any()
            for rule in (brisk_amd.select_rule("solid_run"), brisk_amd.select_rule("median", lo=2, hi=40)):
                d_iv = torch.full((max(n_reads, 1) * 8,), 0x77, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ix.select_intervals(d_prof.data_ptr(), n_reads, rule, d_iv.data_ptr())
                iv, want_iv = d_iv.cpu().numpy().view(brisk_amd.READ_INTERVAL_DTYPE)[:n_reads], brisk_amd.intervals_from_profile(prof, ix.k, rule)
                assert np.array_equal(iv, want_iv), (what, "rule", rule.kind)
                assert (want_iv["len"] > 0).any() and (want_iv["len"] == 0).any()


def fill(B, reads, k, m, b, n_owners, count_mode=None):
    """sharded_job.run without its checks against the oracle's digest (whose counts wrap: a saturating job that passes 255 differs):
    an open Job whose owners hold `reads`"""
    import torch
    job = S.Job(B, k, m, b, n_owners, None, 0, count_mode)
    try:
        W = job.owners[0].record_words
        inbox, slices = S.scan_all(job, reads)
        for ix, recv, sl in zip(job.owners, inbox, slices):
            torch.cuda.synchronize()
            n = recv.numel() // W
            ix.insert_records_hist(recv.data_ptr() if n else 0, n, sl.data_ptr() if sl.numel() else 0, n_owners)
            ix.sync()
        job.reads = list(reads)
        return job
    except Exception:
        job.close()
        raise


def check_case(B, reads, queries, k, m, b, n_owners, profiles=False, **kw):
    """one job: count `reads` on n_owners owners, ask for every k-mer of `queries`, compare with the oracle; with `profiles` also
    the reductions over the placed slots.  Returns the slots."""
    from test_kmer_query import assert_slots
    want, alts, base = expected(reads, queries, k, m, b)
    with S.run(B, reads, k, m, b, n_owners, **kw) as job:
        t = round_trip(job, queries)
        assert_slots(t.slots, want, alts, (k, m, b, n_owners, kw))
        if profiles:
            check_profiles(job.owners[-1], t, resolved(want, alts, t.slots), base, len(queries), (k, m, b))
        return t.slots
