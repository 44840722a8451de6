"""One driver for an N-owner job on ONE device, shared by tests/test_sharded.py, tests/test_sharded_cpu.py,
tests/sharded_variant_worker.py and tests/sharded_ranks_worker.py; their inputs are in tests/sharded_cases.py.  Nothing here is a test.

run() plays every rank of a sharded count in turn through the C-ABI -- scan_packed, route_records, export_hist / export_hist_add on
the scanning side, insert_records_hist / insert_records on the owner -- and get() the query round trip (scan_query, route_tagged,
query_records, index_add_ by tag).  On the way both assert what must hold of the routed records whatever the index later says,
each invariant computed in numpy from the records themselves:

  range          every record routed to owner o lies in [cut[o], cut[o + 1]); partition = (header & 0xffffffff) >> (2b + ext_bits -
                 part_bits); for equal ranges the cuts are exchange.uniform_cuts
  conservation   route_records' per-owner counts are np.bincount of those owners; the multiset of routed records is the multiset
                 of scanned records (for the get: of (tag, record) pairs)
  histogram      the exported histogram is np.add.at(hist, partition, 1 + (n << 32)) over the scanned records, partition by
                 partition (also when the scan threw its own away and rebuilt it); partitions_per_owner = the differences of the cuts
  disjointness   no entry identity on two owners
  checksums      the owners' checksum() add up (digests modulo 2^64) to oracle.digest of the oracle's index of the same reads

Expected values are the oracle's, or numpy over records this module holds; nothing is computed by the library under test."""
import numpy as np

import oracle

M32 = np.uint64(0xffffffff)
_O = None
_expect = {}
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def the_oracle():
    global _O
    if _O is None:
        oracle.build(ref=False)
        _O = oracle.Oracle()
    return _O


# ---- owner arithmetic (tests/test_sharded_cpu.py holds it against brisk_amd.exchange) ------------------------------------------
def owner_of(part, cuts):
    """owner of partition(s) under cut points: the number of owners after the first whose range starts at or below the partition"""
    part = np.asarray(part, dtype=np.int64)
    inner = np.asarray(cuts[1:-1], dtype=np.int64)
    return (part[..., None] >= inner).sum(axis=-1).astype(np.int64) if len(inner) else np.zeros(part.shape, np.int64)


def routing_shift(lay, b):
    return 2 * b + lay["ext_bits"] - lay["part_bits"]


def partitions(rec, lay, b):
    """partition of every record (rows of record_words u64, header last)"""
    return ((rec[:, -1] & M32) >> np.uint64(routing_shift(lay, b))).astype(np.int64)


def instances(rec):
    return ((rec[:, -1] >> np.uint64(32)) & np.uint64(0xff)).astype(np.int64)


def sparse_hist(part, n):
    """np.add.at(hist, part, 1 + (n << 32)) without the empty partitions: (partitions, words), ascending"""
    if not len(part):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    uniq, inv = np.unique(part, return_inverse=True)
    words = np.zeros(len(uniq), np.int64)
    np.add.at(words, inv, 1 + (n << 32))
    return uniq, words


def canon(rows):
    """the rows of a 2-d array as a sorted multiset"""
    rows = np.ascontiguousarray(rows)
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows


def same_rows(a, b):
    return a.shape == b.shape and np.array_equal(canon(a), canon(b))


# ---- the oracle's side -------------------------------------------------------------------------------------------------------------
class Expect:
    """the oracle's index of one read set: kept for the life of the process (queries look entries up in it), never changed"""

    def __init__(self, reads, k, m, b):
        O = the_oracle()
        self.k, self.m, self.b = k, m, b
        self.flat, self.offs = oracle.pack_reads(reads)
        self.h = O.index_new(k, m, b)
        O.index_insert_reads(self.h, self.flat, self.offs)
        self.dump = O.index_dump(self.h)
        self.stats = O.index_stats(self.h)  # (nb_kmers, nb_buckets)
        # (oracle.digest is the definition in Python; the C restatement of the same sum serves the large indexes)
        self.digest = oracle.digest(*self.dump) if len(self.dump[0]) <= 40000 else O.index_digest(self.h)
        self._lines = None

    @property
    def lines(self):
        if self._lines is None:
            self._lines = oracle.multiset_lines(*self.dump, self.k)
        return self._lines

    def entries(self):
        return entry_rows(*self.dump)

    def query(self, queries):
        qf, qo = oracle.pack_reads(queries)
        return the_oracle().index_query_reads(self.h, qf, qo)


def expect(reads, k, m, b):
    key = (k, m, b, hash(tuple(reads)), len(reads))
    if key not in _expect:
        _expect[key] = Expect(reads, k, m, b)
    return _expect[key]


def entry_rows(lo, hi, idx, cnt):
    """entries as sorted rows (hi, lo, idx, count)"""
    return canon(np.stack([np.asarray(hi, np.uint64), np.asarray(lo, np.uint64), np.asarray(idx).astype(np.uint64), np.asarray(cnt).astype(np.uint64)], axis=1))


def cls_env():
    """BRISK_CLS_BITS as the library of this process reads it: -1 when unset"""
    import os
    return int(os.environ.get("BRISK_CLS_BITS", -1))


def layout_of(k, m, b, part_bits=0, cls_env=-1):
    from geometry_edges import layout
    return layout(k, m, b, part_bits, cls_env)


def oracle_pieces(reads, k, m, b, lay):
    """What the scan must emit for `reads`, from the oracle's super-k-mer records alone: per record piece its routing id and its
    k-mers, and per k-mer its identity -- arrays (rid, n) per piece and (rid, compacted, idx') per k-mer.  The routing id is the
    bucket id, then the layout's hash bits -- the low bits of what the compacted k-mer keeps of the hashed minimizer: (m - b)
    nucleotides at the minimizer's offset -- then the class of minimizer_idx; a super-k-mer is cut where the class changes."""
    O = the_oracle()
    sr, cls, width = (m - b + 1) // 2, lay["cls_bits"], lay["cls_width"]
    he, top = lay["ext_bits"] - cls, (1 << cls) - 1
    ones, rest_mask = (1 << (2 * (k - b))) - 1, (1 << (2 * (m - b))) - 1
    h = O.index_new(k, m, b)
    rid_n, kmers = [], []
    for s in reads:
        C, bucket, n, idx0 = O.records(h, s, k, m, b)
        for i in range(len(n)):
            Cv = sum(int(w) << (64 * j) for j, w in enumerate(C[i]))
            ni, first = int(n[i]), int(idx0[i]) - sr  # minimizer_idx of element 0; it rises by one per element
            rest = (Cv >> (2 * (first + ni - 1))) & rest_mask  # read off the last element, which lies at offset 0
            base = (int(bucket[i]) << he) | (rest & ((1 << he) - 1))
            j0 = 0
            while j0 < ni:
                c = min((first + j0) // width, top) if cls else 0
                j1 = ni if not cls or c == top else min(ni, (c + 1) * width - first)
                rid = (base << cls) | c
                rid_n.append((rid, j1 - j0))
                kmers += [(rid, (Cv >> (2 * (ni - 1 - j))) & ones, first + sr + j) for j in range(j0, j1)]
                j0 = j1
    O.index_free(h)
    return np.array(rid_n, dtype=np.int64).reshape(-1, 2), kmers


def oracle_partitions(reads, k, m, b, part_bits=0, cls_env=-1):
    """(partition, k-mers) of every record piece the scan must emit, from the oracle alone; and the layout"""
    lay = layout_of(k, m, b, part_bits, cls_env)
    pieces, _ = _once(("pieces", k, m, b, part_bits, cls_env, hash(tuple(reads))), lambda: oracle_pieces(reads, k, m, b, lay))
    return pieces[:, 0] >> (2 * b + lay["ext_bits"] - lay["part_bits"]), pieces[:, 1], lay


# ---- the device's side -------------------------------------------------------------------------------------------------------------
def to_device(ix, reads):
    """(d_packed, d_starts) of `reads`: ASCII up, packed on the device"""
    import torch
    flat, offs = oracle.pack_reads(reads)
    d_bases = torch.from_numpy(flat if len(flat) else np.zeros(1, np.uint8)).cuda()
    d_packed = torch.zeros((len(flat) + 15) // 16 + 4, dtype=torch.int32, device="cuda")
    d_starts = torch.from_numpy(offs.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    if len(flat):
        ix.pack_ascii(d_bases.data_ptr(), len(flat), d_packed.data_ptr())
    ix.sync()
    return d_packed, d_starts


def host_rows(t, n, W):
    return t[: n * W].cpu().numpy().view(np.uint64).reshape(n, W)


def check_routed(rec, out, counts, cuts, lay, b, tags=None, tags_out=None):
    """range and conservation of one routing call; returns the owner of every routed record"""
    n_owners = len(cuts) - 1
    counts = [int(c) for c in counts]
    part_in, part_out = partitions(rec, lay, b), partitions(out, lay, b)
    want = np.bincount(owner_of(part_in, cuts), minlength=n_owners)
    assert counts == want.tolist(), ("route: per-owner counts", counts, want.tolist())
    owner_out = np.repeat(np.arange(n_owners), counts)
    lo, hi = np.asarray(cuts[:-1], np.int64)[owner_out], np.asarray(cuts[1:], np.int64)[owner_out]
    bad = (part_out < lo) | (part_out >= hi)
    assert not bad.any(), ("route: %d records outside their owner's range, first at slot %d" % (int(bad.sum()), int(np.argmax(bad))))
    if tags is None:
        assert same_rows(rec, out), "route: the routed records are not the scanned records"
    else:
        pair = lambda r, t: np.concatenate([t.astype(np.uint64)[:, None], r], axis=1)
        assert same_rows(pair(rec, tags), pair(out, tags_out)), "route: a tag left its record"
    return owner_out


def check_hist(d_hist, part, n, lens, cuts, what=""):
    """the exported histogram on the device against the records' own, partition by partition"""
    import torch
    assert [int(v) for v in lens] == [cuts[o + 1] - cuts[o] for o in range(len(cuts) - 1)], ("partitions_per_owner", what)
    uniq, words = sparse_hist(part, n)
    nz = int(torch.count_nonzero(d_hist))
    assert nz == len(uniq), ("histogram: %d partitions counted, the records lie in %d" % (nz, len(uniq)), what)
    if len(uniq):
        got = d_hist[torch.from_numpy(uniq).cuda()].cpu().numpy()
        bad = got != words
        assert not bad.any(), ("histogram: %d partitions differ, first %d: %#x for %#x" % (int(bad.sum()), int(uniq[np.argmax(bad)]), int(got[np.argmax(bad)]), int(words[np.argmax(bad)])), what)


def scan_route(ix, d_packed, d_starts, lo, hi, cuts, b, d_acc, add, seen):
    """one piece of one rank: scan reads [lo, hi), route, export; asserts range, conservation and histogram.  `seen` collects the
    (partition, n) of everything scanned into d_acc so far.  Returns (routed records on the device, counts, lens, scanned rows)."""
    import torch
    W, lay = ix.record_words, ix.layout
    st = d_starts[lo:hi + 1].contiguous()
    bound = ix.scan_bound(st.data_ptr(), hi - lo)
    d_rec = torch.zeros(max(bound, 1) * W, dtype=torch.int64, device="cuda")
    d_out = torch.zeros_like(d_rec)
    torch.cuda.synchronize()
    n_rec = ix.scan_packed(d_packed.data_ptr(), st.data_ptr(), hi - lo, d_rec.data_ptr(), bound)
    counts = ix.route_records(d_rec.data_ptr(), n_rec, d_out.data_ptr())
    lens = ix.export_hist_add(d_acc.data_ptr()) if add else ix.export_hist(d_acc.data_ptr())
    ix.sync()
    assert int(counts.sum()) == n_rec
    rec, out = host_rows(d_rec, n_rec, W), host_rows(d_out, n_rec, W)
    check_routed(rec, out, counts, cuts, lay, b)
    if not add:
        del seen[:]
    seen.append((partitions(rec, lay, b), instances(rec)))
    check_hist(d_acc, np.concatenate([p for p, _ in seen]), np.concatenate([n for _, n in seen]), lens, cuts, (lo, hi))
    return d_out, [int(c) for c in counts], [int(v) for v in lens], rec


class Job:
    """the owners of one sharded job, open until close(): .owners, .cuts (as routed by), .layout, .reads (everything counted so far),
    .records (the scanned records of the last run, all ranks), and per owner .lines(), .stats, .checksums"""

    def __init__(self, B, k, m, b, n_owners, cuts, part_bits, count_mode):
        kw = dict(part_bits=part_bits)
        if count_mode is not None:
            kw["count_mode"] = count_mode
        self.k, self.m, self.b, self.part_bits = k, m, b, part_bits
        self.owners = []
        try:
            for r in range(n_owners):
                self.owners.append(B.BriskHip(k, m, b, owner_rank=r, n_owners=n_owners, **kw))
            self.layout = self.owners[0].layout
            if cuts is not None:
                for ix in self.owners:
                    ix.set_owner_cuts(cuts)
        except Exception:
            self.close()
            raise
        from brisk_amd.exchange import uniform_cuts
        self.cuts = [int(c) for c in cuts] if cuts is not None else uniform_cuts(self.layout["part_bits"], n_owners)
        self.reads, self.records = [], None

    def close(self):
        for ix in self.owners:
            ix.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def collect(self):
        self.dumps = [ix.enumerate() for ix in self.owners]
        self.stats = [ix.stats() for ix in self.owners]
        self.checksums = [ix.checksum() for ix in self.owners]
        # disjointness: an entry's identity is (k-mer, minimizer_idx)
        ident = np.concatenate([np.stack([d[1], d[0], d[2].astype(np.uint64)], axis=1) for d in self.dumps])
        assert len(np.unique(ident, axis=0)) == len(ident), "an entry identity appears on two owners"
        for d, st, cs in zip(self.dumps, self.stats, self.checksums):
            assert len(d[0]) == st["nb_kmers"] == cs[0]
        # (the oracle's counts wrap at 256: a saturating job is held to them too, so its reads must keep every count below 255)
        want = expect(self.reads, self.k, self.m, self.b).digest
        got = (sum(c[0] for c in self.checksums), sum(c[1] for c in self.checksums), sum(c[2] for c in self.checksums) % (1 << 64))
        assert got == want, ("the owners' checksums do not add up to the oracle's digest", got, want)

    def lines(self, o=None):
        """sorted multiset lines of owner o, or of all owners together"""
        ds = self.dumps if o is None else [self.dumps[o]]
        return sorted(l for d in ds for l in oracle.multiset_lines(*d, self.k))

    def entries(self):
        return entry_rows(*[np.concatenate([d[i] for d in self.dumps]) for i in range(4)])

    def check(self, lines=True):
        """The owners together hold the oracle's index of everything counted so far: entries (as lines, or as rows for a large
        index), nb_kmers, and nb_buckets owner by owner -- the distinct buckets among the oracle's records of the owner's range.
        Those add up to the oracle's nb_buckets where no owner boundary cuts a bucket: always without ext_bits (a partition is a
        range of whole buckets), and with ext_bits (one bucket is 2^ext_bits partitions) when every cut is a multiple of that."""
        E = expect(self.reads, self.k, self.m, self.b)
        if lines:
            assert self.lines() == E.lines, "the owners' entries are not the oracle's"
        else:
            assert np.array_equal(self.entries(), E.entries()), "the owners' entries are not the oracle's"
        assert sum(s["nb_kmers"] for s in self.stats) == E.stats[0]
        ext = self.layout["ext_bits"]
        part, _, _ = oracle_partitions(self.reads, self.k, self.m, self.b, self.part_bits, cls_env())
        owner, bucket = owner_of(part, self.cuts), part >> ext if ext else None
        want = [len(set(bucket[owner == o].tolist())) for o in range(len(self.owners))] if ext else None
        got = [s["nb_buckets"] for s in self.stats]
        if ext:
            assert got == want, ("nb_buckets per owner", got, want)
        if not ext or all(c % (1 << ext) == 0 for c in self.cuts):
            assert sum(got) == E.stats[1], ("nb_buckets", got, E.stats[1])
        else:
            assert sum(got) >= E.stats[1]
        return E


def scan_all(job, reads, pieces=1):
    """the scanning side of one batch: every rank scans its share and routes it.  Returns per owner what it is handed: its records
    (one tensor, grouped by source rank) and the ranks' histogram slices of its range, side by side."""
    import torch
    owners, lay, cuts, b = job.owners, job.layout, job.cuts, job.b
    n_owners, W, n_parts = len(owners), owners[0].record_words, 1 << lay["part_bits"]
    assert cuts[0] == 0 and cuts[-1] == n_parts and len(cuts) == n_owners + 1
    d_packed, d_starts = to_device(owners[0], reads)
    share = [len(reads) * i // n_owners for i in range(n_owners + 1)]
    inbox, slices, scanned = [[] for _ in owners], [[] for _ in owners], []
    d_acc = torch.zeros(n_parts, dtype=torch.int64, device="cuda")
    for r, ix in enumerate(owners):
        d_acc.zero_()
        seen, lens = [], None
        edges = [share[r] + (share[r + 1] - share[r]) * i // pieces for i in range(pieces + 1)]
        for lo, hi in zip(edges[:-1], edges[1:]):
            d_out, counts, lens, rec = scan_route(ix, d_packed, d_starts, lo, hi, cuts, b, d_acc, pieces > 1, seen)
            scanned.append(rec)
            at = 0
            for o in range(n_owners):
                inbox[o].append(d_out[at * W:(at + counts[o]) * W].clone())
                at += counts[o]
        for o in range(n_owners):  # one slice per owner and rank, summed over the rank's pieces
            slices[o].append(d_acc[cuts[o]:cuts[o + 1]].clone())
    job.records = np.concatenate(scanned)
    return [torch.cat(x) for x in inbox], [torch.cat(x) for x in slices]


def entry_partitions(E, reads, part_bits=0, cls_env=-1):
    """The partition of every entry of the oracle's index E of `reads` (in index_dump's order), from the oracle alone: the
    enumerator stream of a read (Oracle.enumerate: the identity (k-mer, minimizer_idx) of every k-mer, super-k-mer by super-k-mer)
    and its records (oracle_pieces: the routing id of every k-mer) list the same k-mers in the same order.  An identity has one
    routing id wherever it occurs."""
    O = the_oracle()
    lay = layout_of(E.k, E.m, E.b, part_bits, cls_env)
    _, kmers = oracle_pieces(reads, E.k, E.m, E.b, lay)
    shift, at, rid_of = 2 * E.b + lay["ext_bits"] - lay["part_bits"], 0, {}
    for s in reads:
        s = s.decode() if isinstance(s, bytes) else s
        if len(s) < E.k:
            continue
        _, _, lo, hi, idx, _ = O.enumerate(s.upper(), E.k, E.m)
        assert len(lo) == len(s) - E.k + 1
        for ident, (rid, _, _) in zip(zip(lo.tolist(), hi.tolist(), idx.tolist()), kmers[at:at + len(lo)]):
            assert rid_of.setdefault(ident, rid) == rid, "one identity, two routing ids"
        at += len(lo)
    assert at == len(kmers)
    return np.array([rid_of[ident] for ident in zip(E.dump[0].tolist(), E.dump[1].tolist(), E.dump[2].tolist())], np.int64) >> shift


def cuts_at_records(part, part_bits, n_owners):
    """cut points that deal the records of partitions `part` out evenly and fall ON partitions that hold records: a cut that
    no record touches cannot tell `cut <= partition` from `cut < partition`"""
    s = np.sort(np.asarray(part, np.int64))
    cuts = [0]
    for o in range(1, n_owners):
        cuts.append(max(cuts[-1], int(s[len(s) * o // n_owners]) if len(s) else 0))
    return cuts + [1 << part_bits]


def job_histogram(B, reads, k, m, b, part_bits=0):
    """the partition histogram of the whole job, from one unsharded scan (checked against the records like every other)"""
    import torch
    with B.BriskHip(k, m, b, part_bits=part_bits) as one:
        d_packed, d_starts = to_device(one, reads)
        pb = one.layout["part_bits"]
        d_hist = torch.zeros(1 << pb, dtype=torch.int64, device="cuda")
        scan_route(one, d_packed, d_starts, 0, len(reads), [0, 1 << pb], b, d_hist, False, [])
    return d_hist, pb


def run(B, reads, k, m, b, n_owners, *, cuts=None, part_bits=0, pieces=1, with_hist=True, count_mode=None, job=None):
    """Count `reads` on n_owners owners of one device: "rank" r scans its contiguous share in `pieces` pieces, every owner gets its
    records (and, with_hist, the ranks' histogram slices of its range).  `job`: a Job to go on with (a second batch).  Returns the
    Job, its owners open and collected; the invariants of the module's docstring are asserted on the way."""
    import torch
    assert torch.cuda.is_available()
    job = job or Job(B, k, m, b, n_owners, cuts, part_bits, count_mode)
    try:
        owners, cuts, W = job.owners, job.cuts, job.owners[0].record_words
        inbox, slices = scan_all(job, reads, pieces)
        for o, ix in enumerate(owners):
            recv, sl = inbox[o], slices[o]
            torch.cuda.synchronize()
            n = recv.numel() // W
            if cuts[o + 1] == cuts[o]:
                assert n == 0, "an owner without partitions received records"
            if with_hist:
                ix.insert_records_hist(recv.data_ptr() if n else 0, n, sl.data_ptr() if sl.numel() else 0, n_owners)
            else:
                ix.insert_records(recv.data_ptr() if n else 0, n)
            ix.sync()
        job.reads = job.reads + list(reads)
        job.collect()
        return job
    except Exception:
        job.close()
        raise


def get(B, job, queries):
    """The query round trip over the open owners of a Job: scan_query and route_tagged on owner 0's handle, query_records on each owner,
    the sums folded per read by tag.  Asserts range and conservation of the routing with the tags: the multiset of (tag, record)
    pairs is unchanged.  Returns the per-read sums (uint64)."""
    import torch
    owners, cuts = job.owners, job.cuts
    ix0 = owners[0]
    W, lay = ix0.record_words, ix0.layout
    d_packed, d_starts = to_device(ix0, queries)
    n = len(queries)
    bound = ix0.scan_bound(d_starts.data_ptr(), n)
    d_rec = torch.zeros(max(bound, 1) * W, dtype=torch.int64, device="cuda")
    d_out = torch.zeros_like(d_rec)
    d_tags = torch.zeros(max(bound, 1), dtype=torch.int32, device="cuda")
    d_tags_out = torch.zeros_like(d_tags)
    torch.cuda.synchronize()
    nq = ix0.scan_query(d_packed.data_ptr(), d_starts.data_ptr(), n, d_rec.data_ptr(), d_tags.data_ptr(), bound)
    counts = [int(c) for c in ix0.route_tagged(d_rec.data_ptr(), d_tags.data_ptr(), nq, d_out.data_ptr(), d_tags_out.data_ptr())]
    ix0.sync()
    assert sum(counts) == nq
    tags, tags_out = d_tags[:nq].cpu().numpy().view(np.uint32), d_tags_out[:nq].cpu().numpy().view(np.uint32)
    assert nq == 0 or int(tags.max()) < n
    check_routed(host_rows(d_rec, nq, W), host_rows(d_out, nq, W), counts, cuts, lay, ix0.b, tags, tags_out)
    sums = torch.zeros(max(nq, 1), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    at = 0
    for o, ix in enumerate(owners):
        if counts[o]:
            ix.query_records(d_out.data_ptr() + at * W * 8, counts[o], sums.data_ptr() + at * 8)
        at += counts[o]
    torch.cuda.synchronize()
    per_read = torch.zeros(n, dtype=torch.int64, device="cuda")
    if nq:
        per_read.index_add_(0, d_tags_out[:nq].to(torch.int64), sums[:nq])
    return per_read.cpu().numpy().astype(np.uint64)
