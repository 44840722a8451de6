"""The device checks of tests/test_sibling_keys.py that also run under kernel variants, and their worker: one process per
environment (the library reads BRISK_BINS, BRISK_INSERT_GENERIC, ... once), the insert and the index-of-X checks over the eight
geometries with compile-time bodies.  Before every step the worker writes `[sibling] stage <geometry> <step>` to stderr, so that the
parent can tell which `[brisk_hip] path:` and `body:` lines (BRISK_TRACE=1) belong to it.  Prints "ok <n checks>".

Every expectation is the oracle's (tests/sibling_keys.Case); everything is compared bit for bit."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

import sibling_keys as S
from index_model import diff_entries


def check_is(O, ix, c, model, what):
    """the index holds exactly the model's entries: the enumerated multiset, nb_kmers, nb_buckets and the checksum"""
    msg = diff_entries(ix.enumerate(), model)
    assert msg is None, (S.geo_id(c.g), what, msg)
    st = ix.stats()
    assert (st["nb_kmers"], st["nb_buckets"]) == model.stats(O, c.hx), (S.geo_id(c.g), what, st)
    assert ix.checksum() == model.digest(O), (S.geo_id(c.g), what)


def check_insert(O, c, ix, mode="wrap"):
    """X + Y in one fresh batch: a sibling must be an entry of its own, in the partition of its sibling"""
    ix.clear()
    ix.insert_reads(c.x + c.y)
    check_is(O, ix, c, c.model(mode, c.dx, c.dy), "X + Y in one batch")
    return 3


def check_gets(ix, c, sums, slots, alts, what, packed=True):
    from test_kmer_query import as_u16, assert_slots, packed_on_device
    gid = S.geo_id(c.g)
    got = ix.get_reads(c.queries)
    assert np.array_equal(got, sums), (gid, what, "get_reads", np.nonzero(got != sums)[0][:5], got[got != sums][:5], sums[got != sums][:5])
    if packed:
        import torch
        d_packed, d_starts, _ = packed_on_device(ix, c.queries)
        d_sums = torch.full((len(c.queries),), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ix.get_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(c.queries), d_sums.data_ptr())
        ix.sync()
        assert np.array_equal(d_sums.cpu().numpy().astype(np.uint64), sums), (gid, what, "get_packed")
    counts, found, base = ix.get_kmers(c.queries)
    assert np.array_equal(base, c.base), (gid, what)
    assert_slots(as_u16(counts, found), slots, alts, (gid, what, "get_kmers"))


def check_index_of_x(O, c, ix):
    """the index of X alone, asked about Y: the primed member of a pair is absent -- sum 0, every slot 0, lookup finds nothing --
    though its key differs from a present entry's in the routing field only (a sibling) or not at all (a cousin)"""
    gid = S.geo_id(c.g)
    ix.clear()
    ix.insert_reads(c.x)
    check_gets(ix, c, c.sums_x, c.slots_x, c.alts_x, "index of X")
    n = len(c.pairs)
    got = ix.get_reads(c.queries[:n])
    assert not got.any(), (gid, "a primed member was found", [c.pairs[i] for i in np.nonzero(got)[0][:3]])
    for d, what in ((c.dy, "Y's identities"), (c.dx, "X's identities")):
        keys = sorted(d)
        data, found = ix.lookup(np.array([x[1] for x in keys], np.uint64), np.array([x[0] for x in keys], np.uint64), np.array([x[2] for x in keys], np.uint8))
        want = np.array([x in c.dx for x in keys])
        bad = np.nonzero(found.astype(bool) != want)[0]
        assert not len(bad), (gid, "lookup of " + what, len(bad), [keys[i] for i in bad[:3]])
        assert np.array_equal(data[want], np.array([c.dx[x] for x in keys if x in c.dx], np.uint8)), (gid, "lookup of " + what)
    return 6


# ---- what the trace must say ---------------------------------------------------------------------------------------------------------
def insert_body(g, generic=False, big=False, lean=False, mode="wrap"):
    """the `body:` line of an insert of geometry g: the instantiation <nw, k - b, shift> of its own part_bits, or <0,0,0>, the
    run-time body"""
    L = S.geo_layout(g)
    args = "0,0,0" if generic else "%d,%d,%d" % (L["nw"], g.k - g.b, L["shift"])
    kernel = "k_insert_first" if lean else "k_insert_big" if big else "k_insert" if generic else "k_insert_fast"
    return "body: %s<%s,%s>" % (kernel, args, mode) + (", then k_insert_fast_listed" if lean else "")


def query_body(g, generic=False, ent=None):
    L = S.geo_layout(g)
    if generic:
        return "body: k_query (run-time body)"
    return "body: k_query_fast<%d,%d,%d," % (L["nw"], g.k - g.b, L["shift"]) + ("%d>" % ent if ent else "")  # (a prefix when the table size is the library's choice)


def is_lean_geometry(g):
    return (g.k, g.m, g.b) == (63, 21, 14)  # k_insert_first exists for <3,49,1..4>


def main():
    import torch  # (before the library: both then share one HIP runtime)
    import brisk_amd
    import oracle
    oracle.build(ref=False)
    O = oracle.Oracle()
    checks = 0
    # With bins forced every insert call completes before it returns: a small batch is deferred otherwise, and its flush takes the
    # classic layout whatever BRISK_BINS says -- the binned scan would only run for the gets.
    immediate = int(os.environ.get("BRISK_BINS", "0")) > 0
    for g in S.BODIES:
        c = S.case(O, g)
        c.preconditions()
        gid = S.geo_id(g)
        with brisk_amd.BriskHip(g.k, g.m, g.b, immediate_inserts=immediate, **({"part_bits": g.part_bits} if g.part_bits else {})) as ix:
            L = S.geo_layout(g)
            assert ix.layout["part_bits"] == L["part_bits"] and torch.cuda.is_available(), (gid, ix.layout)
            print("[sibling] stage %s insert" % gid, file=sys.stderr, flush=True)
            checks += check_insert(O, c, ix)
            print("[sibling] stage %s index-of-x" % gid, file=sys.stderr, flush=True)
            checks += check_index_of_x(O, c, ix)
            print("[sibling] stage %s done" % gid, file=sys.stderr, flush=True)
    print("ok", checks)


if __name__ == "__main__":
    main()
