"""Worker of test_geometry_edges.py's kernel-variant and BRISK_CLS_BITS tests: one process per environment (the library reads
BRISK_BINS, BRISK_HUGE_AT, BRISK_HUGE_QUERY_AT, BRISK_DEFER and BRISK_CLS_BITS once), the device paths against the oracle at the
rows of tests/geometry_edges.py.  Prints "ok <n checks>"; any mismatch is an AssertionError and exit status 1.

  variants   every row: insert in two batches, get_reads, get_kmers, one merge; "variants corners": the same over
             geometry_edges.CORNERS
  cls        the class rows and (31, 11, 11), (63, 11, 4): layout, index, get_reads, get_kmers, the scan's records element by
             element and every record within one class; a snapshot of this setting is written to GEOMETRY_WORKER_DIR/child-<row>.snap
             and the parent's file (parent-<row>.snap) is loaded: refused with EINVAL unless it was saved under the same cls_bits"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # before the library: torch's HIP runtime first, as in the test process

import brisk_amd
import geometry_edges as G
import oracle
from test_kmer_query import as_u16, assert_slots
from test_setops import as_dump, expected
from test_spectrum_prune import same_multiset, want_stats

EINVAL = 1


def check_is(O, ix, h, want, what):
    assert same_multiset(ix.enumerate(), want), what
    assert ix.checksum() == O.digest_entries(*want), what
    st = ix.stats()
    assert (st["nb_kmers"], st["nb_buckets"]) == want_stats(O, h, want), what


def filled(r, reads):
    ix = brisk_amd.BriskHip(r.k, r.m, r.b, **G.opts(r))
    half = len(reads) // 2
    ix.insert_reads(reads[:half])
    ix.insert_reads(reads[half:])
    return ix


def index_and_gets(O, r, c, ix):
    what = G.row_id(r)
    check_is(O, ix, c.ha, c.dump_a, (what, "index"))
    assert np.array_equal(ix.get_reads(c.queries), c.sums), (what, "get_reads")
    counts, found, base = ix.get_kmers(c.queries)
    assert np.array_equal(base, c.base), (what, "slot bases")
    assert_slots(as_u16(counts, found), c.slots, c.alts, (what, "get_kmers"))
    return 3


def variants(O, rows=G.TABLE):
    checks = 0
    for r in rows:
        c = G.case(O, r)
        with filled(r, c.reads_a) as ix, filled(r, c.reads_b) as src:
            G.check_library_layout(r, ix.layout)
            checks += 1 + index_and_gets(O, r, c, ix)
            want = expected("merge", c.da, c.db)
            assert ix.merge(src) == len(want) - len(c.da), (G.row_id(r), "merge")
            check_is(O, ix, c.ha, as_dump(want), (G.row_id(r), "merge"))
            checks += 1
    return checks


def scan_records(ix, reads):
    """the scan's records of `reads`: (rows of record_words u64, record_words)"""
    flat, offs = oracle.pack_reads(reads)
    d_bases = torch.from_numpy(flat).cuda()
    d_packed = torch.zeros((len(flat) + 15) // 16 + 4, dtype=torch.int32, device="cuda")
    d_starts = torch.from_numpy(offs.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    ix.pack_ascii(d_bases.data_ptr(), len(flat), d_packed.data_ptr())
    bound = ix.scan_bound(d_starts.data_ptr(), len(reads))
    assert bound == sum(max(0, len(s) - ix.k + 1) for s in reads)
    W = ix.record_words
    d_rec = torch.zeros(max(bound, 1) * W, dtype=torch.int64, device="cuda")
    n_rec = ix.scan_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(reads), d_rec.data_ptr(), bound)
    ix.sync()
    return d_rec.cpu().numpy().view(np.uint64)[: n_rec * W].reshape(n_rec, W), W


def records_match(O, r, c, ix):
    """the property of test_gpu_parity.test_scan_records_match_oracle_records: the oracle's k-mers element by element, and every
    record within one class of minimizer_idx"""
    k, m, b = r.k, r.m, r.b
    reads = c.queries
    want, _ = G.oracle_records(O, c.ha, reads, r)
    rec, W = scan_records(ix, reads)
    lay = ix.layout
    ext = lay["ext_bits"]
    got = [tuple(int(x) for x in row[: W - 1]) + ((int(row[W - 1]) & 0xffffffff) >> ext, (int(row[W - 1]) >> 32) & 0xff, (int(row[W - 1]) >> 40) & 0xff) for row in rec]
    if not lay["cls_bits"]:
        assert sorted(got) == sorted(want), (G.row_id(r), "records")
        return
    assert sorted(G.record_elements(got, W, k, b)) == sorted(G.record_elements(want, W, k, b)), (G.row_id(r), "record elements")
    top, width, sr = (1 << lay["cls_bits"]) - 1, lay["cls_width"], (m - b + 1) // 2
    assert len(got) > len(want), (G.row_id(r), "no super-k-mer was cut")
    for row, t in zip(rec, got):
        n, idx0 = t[W:]
        classes = {min((idx0 - sr + j) // width, top) for j in range(n)}
        assert classes == {int(row[W - 1]) & top}, (G.row_id(r), "a record spans classes")


def cls(O):
    env = int(os.environ["BRISK_CLS_BITS"])
    folder = os.environ["GEOMETRY_WORKER_DIR"]
    checks = 0
    for r in G.cls_rows():
        c = G.case(O, r)
        with filled(r, c.reads_a) as ix:
            L = G.check_library_layout(r, ix.layout, cls_env=env)
            assert ix.layout["cls_bits"] == min(env, 3)
            checks += 1 + index_and_gets(O, r, c, ix)
            records_match(O, r, c, ix)
            checks += 1
            mine = os.path.join(folder, "child-%s.snap" % G.row_id(r))
            assert ix.save(mine) == len(c.dump_a[0])
            info = brisk_amd.snapshot_info(mine)
            G.check_library_layout(r, ix.layout, info, cls_env=env)
            assert info["key_words"] == L["key_words"]
            checks += 1
        theirs = os.path.join(folder, "parent-%s.snap" % G.row_id(r))
        saved_under = brisk_amd.snapshot_info(theirs)["cls_bits"]
        with brisk_amd.BriskHip(r.k, r.m, r.b) as ld:
            if saved_under == L["cls_bits"]:
                assert ld.load(theirs) == len(c.dump_a[0])
            else:
                try:
                    ld.load(theirs)
                    raise AssertionError((G.row_id(r), "a snapshot saved under cls_bits = %d was loaded under %d" % (saved_under, L["cls_bits"])))
                except brisk_amd.BriskHipError as e:
                    assert e.code == EINVAL and any(f in str(e) for f in ("part_bits", "ext_bits", "cls_bits")), str(e)
                assert ld.checksum() == (0, 0, 0)
        checks += 1
    return checks


if __name__ == "__main__":
    assert torch.cuda.is_available()
    oracle.build(ref=False)
    if sys.argv[1:] == ["variants", "corners"]:
        print("ok", variants(oracle.Oracle(), G.CORNERS))
    else:
        print("ok", {"variants": variants, "cls": cls}[sys.argv[1]](oracle.Oracle()))
