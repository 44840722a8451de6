"""Worker of test_percall_edges.py's environment tests: one process per environment (the library reads BRISK_CLS_BITS, BRISK_NO_VMM,
BRISK_TRACE and BRISK_ARENA_LIMIT when a handle is created), the per-call path against tests/percall_reference.py.  Prints
"ok <n checks>"; any mismatch is an AssertionError and exit status 1.

  cls      the class rows and (31, 11, 11), (63, 11, 4) under BRISK_CLS_BITS: layout, the stream (whole vectors under every setting),
           upsert / find / enumerate_ids and stats
  growth   BRISK_NO_VMM=1 BRISK_TRACE=1, the growth inputs: the arena is copied to the predicted sizes, every id handed out before a
           copy is found after it, the resume path's trace lines name the predicted k-mers, the end state is the oracle's
  limit    the same fill under a BRISK_ARENA_LIMIT that lets the first growth through: the upsert that needs the second answers ENOMEM
           and leaves a prefix of its vector in the index; a handle without the limit takes the same vectors"""
import os
import re
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # before the library: torch's HIP runtime first, as in the test process

import brisk_amd
import geometry_edges as G
import oracle
import percall_reference as P
from test_percall_edges import check_end_state, check_find_all, check_stream, fill

ENOMEM = 4
RESUMED = re.compile(r"\[brisk_hip\] path: upsert resumed behind (\d+) of (\d+) k-mers, arena full at (\d+) of (\d+) entries")


def cls(O):
    env = int(os.environ["BRISK_CLS_BITS"])
    checks = 0
    for r in G.cls_rows():
        rp, what = P.replay(O, r), (G.row_id(r), "cls_bits", env)
        with brisk_amd.BriskHip(r.k, r.m, r.b, entry_ids=True, **G.opts(r)) as ix:
            G.check_library_layout(r, ix.layout, cls_env=env)
            assert ix.layout["cls_bits"] == min(env, 3)
            check_stream(ix, rp, what)
            fill(ix, rp, what)
            check_find_all(ix, rp, what)
            check_end_state(O, ix, rp, r, what)
            checks += 3
    return checks


class Stderr:
    """the process's file descriptor 2 into a file for a while: the library's trace lines"""

    def __enter__(self):
        sys.stderr.flush()
        self.file = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.file.fileno(), 2)
        return self

    def __exit__(self, *a):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.file.seek(0)
        self.text = self.file.read().decode()
        self.file.close()
        sys.stderr.write(self.text)


def entry_bytes(r):
    return 8 * G.row_layout(r)["key_words"] + 1 + 4  # key, count byte, id


def entries_after_vectors(vectors):
    """entries in the index once vector i is in"""
    return np.maximum.accumulate([int(v.ids.max()) + 1 for v in vectors])


def resumes(text):
    return [tuple(int(x) for x in m.groups()) for m in RESUMED.finditer(text)]


def growth(O):
    assert os.environ["BRISK_NO_VMM"] == "1" and os.environ["BRISK_TRACE"] == "1"
    checks = 0
    for r in P.GROWTH_ROWS:
        rp, parts, growths, cursor = P.growth_case(O, r)
        what = (G.row_id(r), "growth")
        sizes = [P.FIRST_ARENA] + [g.arena for g in growths]
        last_of_seq = {v.seq: vi for vi, v in enumerate(rp.vectors)}
        entries_after = entries_after_vectors(rp.vectors)
        seen = [0]

        def after_vector(vi):
            if last_of_seq[rp.vectors[vi].seq] != vi:
                return
            mapped = ix.memory_info()["arena_mapped"]
            if mapped != seen[-1]:  # the arena has moved: every id handed out so far is still found
                assert mapped > seen[-1]
                seen.append(mapped)
                check_find_all(ix, rp, what + ("after the arena grew to", mapped), n=int(entries_after[vi]))

        with Stderr() as err, brisk_amd.BriskHip(r.k, r.m, r.b, entry_ids=True, **G.opts(r)) as ix:
            G.check_library_layout(r, ix.layout)
            assert ix.memory_info()["arena_mapped"] == 0
            fill(ix, rp, what, after_vector)
            check_find_all(ix, rp, what)
            check_end_state(O, ix, rp, r, what)
        rises = seen[1:]
        print(G.row_id(r), "arena_mapped after a sequence:", rises, "predicted entries:", sizes, "resumed:", resumes(err.text))
        assert len(rises) >= 3 and set(rises) <= {s * entry_bytes(r) for s in sizes} and rises[-1] == sizes[-1] * entry_bytes(r), what  # first mapping, two growths
        got = resumes(err.text)
        assert got == [(g.done, g.n, g.used, before) for g, before in zip(growths, sizes)], (what, got, growths)
        assert any(0 < done < n for done, n, _, _ in got), what
        checks += 2
    return checks


def limit(O):
    assert os.environ["BRISK_NO_VMM"] == "1"
    checks = 0
    for r in P.GROWTH_ROWS:
        rp, parts, growths, cursor = P.growth_case(O, r)
        what = (G.row_id(r), "limit")
        refused = P.predict_growths(rp, parts, limit=P.arena_limit(growths))[0][-1]
        assert refused.arena is None and 0 <= refused.done < refused.n
        v = rp.vectors[refused.vector]
        head = types.SimpleNamespace(vectors=rp.vectors[:refused.vector])  # the replay up to the vector that is refused
        os.environ["BRISK_ARENA_LIMIT"] = str(P.arena_limit(growths))
        with Stderr() as err, brisk_amd.BriskHip(r.k, r.m, r.b, entry_ids=True, **G.opts(r)) as ix:
            del os.environ["BRISK_ARENA_LIMIT"]  # (read at create)
            fill(ix, head, what)
            n_before = int(entries_after_vectors(head.vectors)[-1])
            try:
                ix.upsert_kmers(v.lo, v.hi, v.idx)
                raise AssertionError(what + ("the upsert beyond the limit went through",))
            except brisk_amd.BriskHipError as e:
                assert e.code == ENOMEM and "BRISK_ARENA_LIMIT" in str(e), str(e)
            # the first `done` k-mers of the vector are in, the new ones among them under the next dense ids; of the rest, only what was there before
            n_now = n_before + int(v.newly[:refused.done].sum())
            in_now = (np.arange(len(v.ids)) < refused.done) | (v.newly == 0)
            assert np.array_equal(ix.find_kmers(v.lo, v.hi, v.idx), np.where(in_now, v.ids, P.ABSENT).astype(np.uint32)), what
            assert not in_now.all()
            lo, hi, idx, ids = ix.enumerate_ids()
            order = np.argsort(ids)
            assert np.array_equal(ids[order], np.arange(n_now, dtype=np.uint32)), what
            assert all(np.array_equal(a[order], w) for a, w in zip((lo, hi, idx), rp.arrays(n_now))), what
            h = O.index_new(r.k, r.m, r.b)
            nb_buckets = len(np.unique(O.bucket_ids(h, *rp.arrays(n_now))))
            O.index_free(h)
            st = ix.stats()
            assert (st["nb_kmers"], st["nb_buckets"]) == (n_now, nb_buckets), what
            check_find_all(ix, rp, what, n=n_now)
        got = resumes(err.text)
        assert got[-1][:3] == refused[1:4] and len(got) == 2, (what, got, refused)
        checks += 1
        with brisk_amd.BriskHip(r.k, r.m, r.b, entry_ids=True, **G.opts(r)) as ix:  # no limit: the same vectors and the refused one go in
            head.vectors = rp.vectors[:refused.vector + 1]
            fill(ix, head, what + ("no limit",))
            check_find_all(ix, rp, what + ("no limit",), n=int(entries_after_vectors(head.vectors)[-1]))
        print(G.row_id(r), "limit", P.arena_limit(growths), "refused:", refused, "entries:", n_now)
        checks += 1
    return checks


if __name__ == "__main__":
    assert torch.cuda.is_available()
    oracle.build(ref=False)
    print("ok", {"cls": cls, "growth": growth, "limit": limit}[sys.argv[1]](oracle.Oracle()))
