"""GPU: sibling keys -- entries that differ only in the routing bits of their key ("sibling keys").

tests/golden/sibling_pairs.json.gz holds pairs of reads whose records are equal word for word apart from the bucket
(tests/sibling_keys.py builds them on the CPU from the oracle alone; tests/test_sibling_keys_cpu.py re-verifies them).  A sibling
pair lies in one partition with keys that differ in the routing field only; a cousin pair has one key in two partitions.  Code that
dropped, misplaced or cut the field -- cut_key, its twin in the query, make_key, the fold's header compare, k_insert_first's 32-bit
proof, either word of a straddling key -- makes one entry of two, or finds an absent k-mer; random reads never hold such a pair.

Per geometry: X = every unprimed member (singles x3, records x2) and 100 random reads, Y = every primed member once and 30 of
those reads.  Expected values are the oracle's (tests/sibling_keys.Case: index_model.batch_dump, index_query_reads, index_get
through test_kmer_query.expected_all) joined by tests/index_model.py; everything is compared bit for bit.  BRISK_TRACE's `path:`
and `body:` lines tell that the intended route and the instantiation of the geometry's own shift ran.

Geometries: the eight with compile-time bodies (k63 m21 b14 at 2^24..2^27 partitions, k31 m15 b14 at 2^24..2^22, k31 m11 b11), the
rows of geometry_edges.TABLE with shift > 0, and two shift-0 rows with cousins only.

Measured on an MI355X: the module takes about 110 s (186 tests).  The longest: the worker of BRISK_BINS=64, 9-11 s (bins of tens of
GB), 5 s for every other worker environment; merge, subtract and the four intersects on the handle of 2^27 partitions, 6 s (every
whole-index call there walks a directory of 512 MB); everything else below 2.5 s."""
import contextlib
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import geometry_edges as G
import oracle
import sibling_keys as S
import sibling_keys_worker as W
import snapshot_reader
from index_model import JOINT_WINDOWS, RULES, diff_entries, expected_slots

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
LEAN = re.compile(r"k_insert_first \(fresh index\): (\d+) partitions lean, (\d+) left over to k_insert, (\d+) partitions to k_insert_huge \((\d+) table-free\)")
INSERT_LINE = "path: insert of"


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


def opts(g):
    return {"part_bits": g.part_bits} if g.part_bits else {}


class Ctx:
    pass


@contextlib.contextmanager
def traced():
    """BRISK_TRACE=1 while handles are created (the library reads it then)"""
    old = os.environ.get("BRISK_TRACE")
    os.environ["BRISK_TRACE"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["BRISK_TRACE"]
        else:
            os.environ["BRISK_TRACE"] = old


@pytest.fixture(scope="module", params=S.GEOMETRIES, ids=[S.geo_id(g) for g in S.GEOMETRIES])
def ctx(request, B, O):
    """one geometry: the oracle's case and two traced handles, made once and reused through clear() (a handle of 2^27 partitions is
    several GB); clear() restores the fresh-index route"""
    g = request.param
    x = Ctx()
    x.g, x.c = g, S.case(O, g)
    x.figures = x.c.preconditions()
    with traced():
        x.a, x.b = B.BriskHip(g.k, g.m, g.b, **opts(g)), B.BriskHip(g.k, g.m, g.b, **opts(g))
    yield x
    x.a.close()
    x.b.close()


def trace(capfd):
    return [l for l in capfd.readouterr().err.splitlines() if l.startswith("[brisk_hip]")]


def body_lines(lines, kind):
    return [l.split("] ", 1)[1] for l in lines if "] body: " + kind in l]


def check_insert_trace(g, lines, first, mode="wrap"):
    """one insert of a batch: `first`: into a fresh index -- at k63 m21 b14 the lean route, with partitions proved duplicate-free;
    else the general body.  The body is the instantiation of the geometry's own shift, the run-time one where there is none."""
    ins = [l for l in lines if INSERT_LINE in l]
    assert len(ins) == 1, lines
    bodies = body_lines(lines, "k_insert")
    assert len(bodies) == 1, lines
    lean = first and W.is_lean_geometry(g)
    m = LEAN.search(ins[0])
    assert bool(m) == lean, ins
    if lean:
        n_lean, n_left, n_huge, n_clean = (int(v) for v in m.groups())
        assert n_lean > 0 and 0 < n_clean <= n_lean, ins
    if g.kind == "body" or (g.k, g.m, g.b) == (31, 11, 11):
        assert bodies[0] == W.insert_body(g, lean=lean, mode=mode), (bodies, W.insert_body(g, lean=lean, mode=mode))
    else:
        assert "<0,0,0,%s>" % mode in bodies[0], bodies


def test_layout(ctx):
    """the handle's layout is the formula's: part_bits, and with it the shift the bodies are instantiated for"""
    L = ctx.c.L
    for f in ("record_words", "part_bits", "ext_bits", "cls_bits", "cls_width"):
        assert ctx.a.layout[f] == L[f], (f, ctx.a.layout, L)


# ---- insert ----------------------------------------------------------------------------------------------------------------------------
def test_insert_one_fresh_batch(ctx, O, capfd):
    trace(capfd)
    W.check_insert(O, ctx.c, ctx.a)
    check_insert_trace(ctx.g, trace(capfd), first=True)


def test_insert_two_batches(ctx, B, O, capfd):
    """the second batch meets its siblings as existing entries: the general body must append an entry, not add to the sibling's count"""
    c, g, a = ctx.c, ctx.g, ctx.a
    for first, second, what in ((c.x, c.y, "X, then Y"), (c.y, c.x, "Y, then X")):
        d1, d2 = (c.dx, c.dy) if first is c.x else (c.dy, c.dx)
        a.clear()
        trace(capfd)
        a.insert_reads(first)
        assert a.checksum() == c.model("wrap", d1).digest(O), what  # (and the first batch is in the index before the second arrives)
        check_insert_trace(g, trace(capfd), first=True)
        a.insert_reads(second)
        W.check_is(O, a, c, c.model("wrap", d1, d2), what)
        check_insert_trace(g, trace(capfd), first=False)
    with traced():
        im = B.BriskHip(g.k, g.m, g.b, immediate_inserts=True, **opts(g))
    with im:
        trace(capfd)
        im.insert_reads(c.x)
        check_insert_trace(g, trace(capfd), first=True)
        im.insert_reads(c.y)
        check_insert_trace(g, trace(capfd), first=False)
        W.check_is(O, im, c, c.model("wrap", c.dx, c.dy), "immediate inserts")


# ---- the index of X, asked about Y ------------------------------------------------------------------------------------------------------
def test_index_of_x(ctx, O, capfd):
    trace(capfd)
    W.check_index_of_x(O, ctx.c, ctx.a)
    bodies = body_lines(trace(capfd), "k_query")
    assert len(bodies) >= 3, bodies  # get_reads, get_packed, get_kmers
    has_body = ctx.g.kind == "body" or (ctx.g.k, ctx.g.m, ctx.g.b) == (31, 11, 11)
    assert all(l.startswith(W.query_body(ctx.g, generic=not has_body)) for l in bodies), (bodies, W.query_body(ctx.g, generic=not has_body))
    assert any("per k-mer" in l for l in bodies) and not all("per k-mer" in l for l in bodies), bodies


# ---- set operations between the index of X and the index of Y ----------------------------------------------------------------------------
def two_indexes(ctx, O, ops):
    """`ops`: [(name, call on the device, call on the model)] with the index of X as the left and the index of Y as the right operand,
    X counted afresh before each; Y's index must be unchanged afterwards, bit for bit"""
    c, a, b = ctx.c, ctx.a, ctx.b
    mx, my = c.model("wrap", c.dx), c.model("wrap", c.dy)
    b.clear()
    b.insert_reads(c.y)
    y_cs, y_entries = b.checksum(), b.enumerate()
    assert y_cs == my.digest(O)
    for what, on_device, on_model in ops:
        a.clear()
        a.insert_reads(c.x)
        want = mx.copy()
        ret = on_model(want, my)
        assert on_device(a, b) == ret, (S.geo_id(ctx.g), what)
        W.check_is(O, a, c, want, what)
        yield what, ret, want
    assert b.checksum() == y_cs and all(np.array_equal(p, q) for p, q in zip(b.enumerate(), y_entries))


def test_compare_and_joint_spectrum(ctx, O):
    c, a, b = ctx.c, ctx.a, ctx.b
    mx, my = c.model("wrap", c.dx), c.model("wrap", c.dy)
    for ix, reads in ((a, c.x), (b, c.y)):
        ix.clear()
        ix.insert_reads(reads)
    want = mx.compare(my)
    assert want["only_other"] == sum(len(ids) for ids in c.ids_b) and want["only_self"] >= sum(len(ids) for ids in c.ids_a)  # no member is shared
    assert a.compare(b) == want and b.compare(a) == my.compare(mx)
    assert np.array_equal(a.joint_spectrum(b), mx.joint_spectrum(my)) and np.array_equal(b.joint_spectrum(a), my.joint_spectrum(mx))
    assert (a.checksum(), b.checksum()) == (mx.digest(O), my.digest(O))


def test_merge_subtract_intersect(ctx, O):
    c = ctx.c
    primed = {x for ids in c.ids_b for x in ids}
    ops = [("merge", lambda ix, o: ix.merge(o), lambda mod, o: mod.merge(o)), ("subtract", lambda ix, o: ix.subtract(o), lambda mod, o: mod.subtract(o))]
    ops += [("intersect " + rule, lambda ix, o, rule=rule: ix.intersect(o, count=rule), lambda mod, o, rule=rule: mod.intersect(o, rule)) for rule in RULES]
    for what, ret, want in two_indexes(ctx, O, ops):
        if what == "merge":  # every primed member arrived as entries of its own, with Y's count
            assert ret == len(primed) and all(want.d[x] == 1 for x in primed)
        elif what == "subtract":  # the unprimed members are not in Y: all of them stay
            assert all(x in want.d for ids in c.ids_a for x in ids)
        else:  # and none of them is in the intersection
            assert not any(x in want.d for ids in c.ids_a for x in ids)


def test_filter_joint(ctx, O):
    """windows: the entries absent from the other index alone; those present in it; count >= 2 here and anything, or absent, there"""
    c = ctx.c
    windows = (JOINT_WINDOWS[1], JOINT_WINDOWS[0], JOINT_WINDOWS[2])
    assert windows[0][4] and windows[0][2] > windows[0][3] and not windows[1][4] and windows[2][4] and windows[2][0] == 2
    ops = [(w, lambda ix, o, w=w: ix.filter_joint(o, *w), lambda mod, o, w=w: mod.filter_joint(o, w)) for w in windows]
    for w, ret, want in two_indexes(ctx, O, ops):
        members = [x for ids in c.ids_a for x in ids]
        assert all(x in want.d for x in members) if w[4] else not any(x in want.d for x in members)


# ---- prune ------------------------------------------------------------------------------------------------------------------------------
def test_prune(ctx, O):
    """X, then Y, then prune(2, 255): the oracle's entries with count >= 2 stay -- of a pair, the unprimed member (3 or 2) stays and
    the primed one (1) goes -- and the gets answer accordingly"""
    c, a = ctx.c, ctx.a
    a.clear()
    a.insert_reads(c.x)
    a.insert_reads(c.y)
    want = c.model("wrap", c.dx, c.dy)
    removed = want.prune(2, 255)
    assert all(x in want.d for ids in c.ids_a for x in ids) and not any(x in want.d for ids in c.ids_b for x in ids) and removed > len(c.pairs)
    assert a.prune(2, 255) == removed
    W.check_is(O, a, c, want, "after prune(2, 255)")
    from test_kmer_query import as_u16, assert_slots
    slots, alts = expected_slots(want, c.slot_ids, c.alt_spans)
    counts, found, base = a.get_kmers(c.queries)
    assert np.array_equal(base, c.base)
    assert_slots(as_u16(counts, found), slots, alts, (S.geo_id(ctx.g), "get_kmers after the prune"))
    # per-read sums: for the reads whose oracle sum over X is the plain sum of their slots and that hold no span equal to its own
    # reverse complement (all of them but a few, asserted), the sum is the sum of the pruned slots
    base_i = c.base.astype(np.int64)
    seg = lambda v: np.array([int(v[base_i[i]:base_i[i + 1]].astype(np.int64).sum()) for i in range(len(c.queries))], np.uint64)
    ambiguous = np.zeros(len(slots), bool)
    for s, e in c.alt_spans:
        ambiguous[s:e] = True
    plain = (seg(c.slots_x & 0xff) == c.sums_x) & (seg(ambiguous) == 0)
    assert plain.mean() > 0.9
    got = a.get_reads(c.queries)
    assert np.array_equal(got[plain], seg(slots & 0xff)[plain])
    n = len(c.pairs)
    assert not got[:n].any() and got[n:2 * n].all()


# ---- snapshot ----------------------------------------------------------------------------------------------------------------------------
def test_snapshot(ctx, B, O, tmp_path):
    c, g, a, b, L = ctx.c, ctx.g, ctx.a, ctx.b, ctx.c.L
    a.clear()
    a.insert_reads(c.x + c.y)
    want = c.model("wrap", c.dx, c.dy)
    path = tmp_path / "xy.snap"
    assert a.save(path) == len(want.d)
    info = B.snapshot_info(path)
    assert (info["part_bits"], info["shift"], info["key_words"]) == (L["part_bits"], L["shift"], L["key_words"]), info
    hdr, blocks = snapshot_reader.read(path)
    assert (hdr["shift"], hdr["part_bits"], hdr["key_words"]) == (L["shift"], L["part_bits"], L["key_words"])

    class Shim:  # what geometry_edges.expected_file_entries reads of a case
        row, ha, reads_a = g, c.hx, c.x + c.y
    got = G.file_entries(blocks, L)
    assert got == G.expected_file_entries(O, Shim, L)
    if L["ext_bits"] == 0:  # the file shows both members of a pair: two keys in one partition (siblings), one key in two (cousins)
        in_file = {}
        for bucket, cls, key, cnt in got:
            in_file[(bucket >> L["shift"], key)] = cnt
        for i, p in enumerate(c.pairs):
            ka, kb = c.file_keys(O, i)
            assert all(in_file.get(x) == (3 if p["size"] == "single" else 2) for x in ka) and all(in_file.get(x) == 1 for x in kb), p
            for (pa, key_a), (pb, key_b) in zip(ka, kb):
                if p["cls"] == "sibling":
                    assert pa == pb and key_a != key_b and (key_a ^ key_b) >> L["entry_bits"] == sum(1 << t for t in p["bits"]), p
                else:
                    assert pa != pb and key_a == key_b, p
    for room in (False, True):
        b.clear()
        assert b.load(path, room=room) == len(want.d)
        W.check_is(O, b, c, want, ("loaded", room))
    W.check_gets(b, c, *gets_of(O, c, want), "loaded, with room", packed=False)


def gets_of(O, c, model):
    """(sums, slots, alts) of the queries against the index holding X + Y: the oracle's own index of those reads"""
    from test_kmer_query import expected_all, oracle_index
    h = oracle_index(O, c.x + c.y, c.g.k, c.g.m, c.g.b)
    try:
        assert diff_entries(O.index_dump(h), model) is None
        slots, alts, _ = expected_all(O, h, c.queries, c.g.k, c.g.m)
        return O.index_query_reads(h, c.qflat, c.qoffs), slots, alts
    finally:
        O.index_free(h)


# ---- reallocate ---------------------------------------------------------------------------------------------------------------------------
REALLOCATE = [g for g in S.GEOMETRIES if g.m + 2 <= 31 and g.m + 2 < g.k and G.layout(g.k, g.m + 2, g.b + 2) is not None]


def test_reallocate_rows():
    """CPU: left out are the rows whose (m + 2, b + 2) is no geometry -- m + 2 = 33 at k33 m31 b14 -- and nothing else"""
    assert [S.geo_id(g) for g in S.GEOMETRIES if g not in REALLOCATE] == ["k33m31b14"]


@pytest.mark.parametrize("g", REALLOCATE, ids=[S.geo_id(g) for g in REALLOCATE])
def test_reallocate(B, O, g):
    """the index of X + Y re-bucketed to (m + 2, b + 2): both members of every pair go through as k-mers of their own"""
    from test_reallocate import _expected, _lines_to_counter
    c = S.case(O, g)
    with B.BriskHip(g.k, g.m, g.b, **opts(g)) as ix, B.BriskHip(g.k, g.m + 2, g.b + 2) as new:
        ix.insert_reads(c.x + c.y)
        before = oracle.multiset_lines(*ix.enumerate(), g.k)
        assert before == oracle.multiset_lines(*c.model("wrap", c.dx, c.dy).dump(), g.k)
        ix.reallocate_into(new)
        after = oracle.multiset_lines(*new.enumerate(), g.k)
    assert _lines_to_counter(after) == _expected(O, before, g.k, g.m + 2)


# ---- saturating counts ----------------------------------------------------------------------------------------------------------------------
def test_saturating_and_wrapping_counts(ctx, B, O):
    """one member 300 times, the other twice: 255 and 2 in a saturating index, 300 - 256 = 44 and 2 in a wrapping one.  An index that
    took the two for one entry would hold 255 (or 46) once."""
    from index_model import as_dict, batch_dump
    c, g = ctx.c, ctx.g
    cls = "sibling" if c.L["shift"] else "cousin"
    chosen = [next(i for i, p in enumerate(c.pairs) if p["cls"] == cls and p["size"] == size) for size in ("single", "record")]
    chosen.append(max(i for i, p in enumerate(c.pairs) if p["cls"] == cls and p["size"] == "record"))  # (a multi-bit pair where there is one)
    first = [c.pairs[i]["a"] for i in chosen] * 200 + [c.pairs[i]["b"] for i in chosen] * 2 + c.bg[:20]
    second = [c.pairs[i]["a"] for i in chosen] * 100
    d_bg = batch_dump(O, c.bg[:20], g.k, g.m, g.b)
    with B.BriskHip(g.k, g.m, g.b, count_mode="saturate", **opts(g)) as sat:
        for ix, big in ((sat, 255), (ctx.a, 44)):
            want = dict(d_bg)
            for i in chosen:
                want.update({x: big for x in c.ids_a[i]})
                want.update({x: 2 for x in c.ids_b[i]})
            ix.clear()
            ix.insert_reads(first)
            assert ix.stats()["nb_kmers"] == len(want)  # (and the first batch is complete before the second)
            ix.insert_reads(second)
            assert as_dict(ix.enumerate()) == want, (S.geo_id(g), big)
            assert ix.checksum() == O.digest_entries(*c.model("wrap", want).dump())


# ---- kernel variants: one process per environment -------------------------------------------------------------------------------------------
VARIANTS = {
    "generic": {"BRISK_INSERT_GENERIC": "1", "BRISK_QUERY_GENERIC": "1", "BRISK_BINS": "0"},
    "bins-0": {"BRISK_BINS": "0"},
    "bins-2": {"BRISK_BINS": "2"},
    "bins-64": {"BRISK_BINS": "64"},
    "lean-off": {"BRISK_INSERT_LEAN": "0"},
    "clean-off": {"BRISK_INSERT_CLEAN": "0"},
    "big": {"BRISK_INSERT_BIG_AT": "0", "BRISK_BINS": "0"},
    "huge": {"BRISK_HUGE_AT": "4", "BRISK_HUGE_QUERY_AT": "0"},
    "query-ent-128": {"BRISK_QUERY_ENT": "128"},
    "query-ent-256": {"BRISK_QUERY_ENT": "256"},
}


@pytest.mark.parametrize("name", list(VARIANTS), ids=["+".join("%s=%s" % kv for kv in env.items()) for env in VARIANTS.values()])
def test_kernel_variants(name):
    """the insert of X + Y and the index-of-X checks over the eight geometries with compile-time bodies (tests/sibling_keys_worker.py),
    and from the trace: the path the environment asks for, in the instantiation of each geometry's own shift"""
    env = {n: v for n, v in os.environ.items() if not n.startswith("BRISK_") or n == "BRISK_HIP_LIB"}
    env.update(VARIANTS[name], BRISK_TRACE="1")
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(TESTS, "sibling_keys_worker.py")], env=env, capture_output=True, text=True, timeout=900)
    print("sibling_keys_worker %s: %.0f s" % (name, time.time() - t0))
    last = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
    assert p.returncode == 0 and last == "ok %d" % (9 * len(S.BODIES)), (name, p.stdout[-3000:], p.stderr[-6000:])
    stages, stage = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("[sibling] stage "):
            stage = tuple(line.split()[2:4])
        elif line.startswith("[brisk_hip]"):
            stages.setdefault(stage, []).append(line)
    for g in S.BODIES:
        gid, L = S.geo_id(g), S.geo_layout(g)
        lines = stages.get((gid, "insert"), [])
        ins = [l for l in lines if INSERT_LINE in l]
        bodies = body_lines(lines, "k_insert")
        assert len(ins) == 1 and len(bodies) == 1, (name, gid, lines)
        generic, big = name == "generic", name == "big"
        lean = W.is_lean_geometry(g) and name not in ("generic", "lean-off", "big")
        assert bodies[0] == W.insert_body(g, generic=generic, big=big, lean=lean), (name, gid, bodies)
        m = LEAN.search(ins[0])
        assert bool(m) == lean, (name, gid, ins)
        if lean:
            n_lean, n_left, n_huge, n_clean = (int(v) for v in m.groups())
            assert n_lean > 0 and (n_clean == 0 if name == "clean-off" else 0 < n_clean <= n_lean), (name, gid, ins)
        if name in ("generic", "bins-0", "big"):
            assert "(classic layout" in ins[0], (name, gid, ins)
        if name == "bins-2" or (name == "bins-64" and L["part_bits"] <= 24):  # (bins of 64 records for 2^25 partitions and more are 64 GB and more, or past
            assert "(binned layout" in ins[0], (name, gid, ins)                # 2^32 slots: the library may fall back to the classic layout there)
        if big:
            assert "k_insert_big" in ins[0], (name, gid, ins)
        huge = int(re.search(r"(\d+) partitions to k_insert_huge", ins[0]).group(1))
        assert (huge > 100) == (name == "huge"), (name, gid, ins)  # (the 150-nt reads and the 8-k-mer records: more than 4 instances each)
        q = body_lines(stages.get((gid, "index-of-x"), []), "k_query")
        assert len(q) >= 3, (name, gid, q)
        want_q = W.query_body(g, generic=generic, ent={"query-ent-128": 128, "query-ent-256": 256}.get(name))
        assert all(l.startswith(want_q) for l in q), (name, gid, q, want_q)

