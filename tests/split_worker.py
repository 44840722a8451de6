"""Worker and shared helpers of test_split.py.  As a program (one process per environment: the library reads BRISK_PROFILE_SEG and
BRISK_PROFILE_BATCH once):
    split_worker.py runs                       brisk_hip_solid_runs over the crafted slot table, against fragments_from_slots
    split_worker.py batches OUT.pkl [MAX]      split_packed and split_reads over error-bearing reads at both geometries (MAX:
                                               max_batch_reads of the handle); the bytes and the stats are left in OUT.pkl
prints "ok <n checks>"."""
import os
import pickle
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # before the library: torch's HIP runtime first, as in the test process

import brisk_amd
from extract_worker import E2E_GEOMETRIES, FILL, device_reads, error_reads
from split_reference import gather_reference, read_lengths, slot_cases

ECAPACITY = 5
SOLID_MINS = (0, 1, 2, 255, 256)
ROW_FILL = 0xA5  # every byte of a fragment buffer before a call


def to_device(a):
    raw = np.ascontiguousarray(a).view(np.uint8)
    t = torch.from_numpy(raw if len(raw) else np.zeros(16, np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


class SplitBuffers:
    """output buffers of one split / solid_runs / extract_fragments call, pre-filled: room for cap_words words and frag_cap rows,
    and a little more that no call may touch"""

    def __init__(self, frag_cap, cap_words=0):
        self.frag_cap, self.cap = frag_cap, cap_words
        self.packed = torch.full((cap_words + 4,), FILL, dtype=torch.int32, device="cuda")
        self.starts = torch.full((frag_cap + 3,), -1, dtype=torch.int64, device="cuda")
        self.frags = torch.full(((frag_cap + 2) * 16,), ROW_FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def host(self):
        torch.cuda.synchronize()
        return (self.packed.cpu().numpy().view(np.uint32), self.starts.cpu().numpy().view(np.uint64), self.frags.cpu().numpy())

    def rows(self, n):
        return self.host()[2][:n * 16].view(brisk_amd.FRAGMENT_DTYPE)

    def untouched(self):
        p, s, f = self.host()
        return bool((p == FILL).all() and (s == np.uint64(0xffffffffffffffff)).all() and (f == ROW_FILL).all())


def slot_words(counts, found):
    """brisk_hip_get_kmers' uint16 slots: 0 absent, 0x100 | count present"""
    return np.where(found, np.uint16(0x100) | counts.astype(np.uint16), np.uint16(0)).astype(np.uint16)


def check_solid_runs(ix, counts, found, base, n_nts, solid_mins=SOLID_MINS):
    """solid_runs over the table against fragments_from_slots, row for row, at every solid_min and min_len: the table, the stats, the
    untouched tail, exactly enough room, and one row too few"""
    k = ix.k
    lens = read_lengths(base, k)
    starts = np.zeros(len(base), np.uint64)
    starts[1:] = np.cumsum(lens, dtype=np.uint64)
    assert int(starts[-1]) == n_nts
    d_slots, d_starts = to_device(slot_words(counts, found)), to_device(starts)
    n_reads, checks = len(base) - 1, 0
    for solid_min in solid_mins:
        for min_len in (0, k, k + 1, k + 7):
            want, want_st = brisk_amd.fragments_from_slots(counts, found, base, k, solid_min, min_len, n_nts_in=n_nts)
            nf = len(want)
            out = SplitBuffers(nf)  # exactly the room it needs
            st = ix.solid_runs(d_slots.data_ptr(), d_starts.data_ptr(), n_reads, out.frags.data_ptr(), nf, solid_min, min_len)
            assert st == want_st, (solid_min, min_len, st, want_st)
            got = out.rows(nf)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (solid_min, min_len, int(bad[0]), got[bad[0]], want[bad[0]])
            p, s, f = out.host()
            assert (f[nf * 16:] == ROW_FILL).all() and (p == FILL).all()  # the tail, and what the call does not write at all
            if nf:
                out = SplitBuffers(nf)
                st = ix.solid_runs(d_slots.data_ptr(), d_starts.data_ptr(), n_reads, out.frags.data_ptr(), nf - 1, solid_min, min_len, raise_on_capacity=False)
                assert st.pop("rc") == ECAPACITY and st == want_st and out.untouched(), (solid_min, min_len)
            checks += 1
    return checks


def crafted_runs(k=31):
    counts, found, base, n_nts = slot_cases(random.Random(2626), k)
    assert len(base) - 1 > 2900 and int(base[1]) == 3 * 4096 + 5
    with brisk_amd.BriskHip(k, 15, 14) as ix:
        return check_solid_runs(ix, counts, found, base, n_nts)


def split_outputs(ix, seqs, solid_min, min_len):
    """split_packed with exactly the room it needs (asked for first) and split_reads: (words, starts, rows, stats, host rows, host stats)"""
    d_packed, d_starts, words, starts = device_reads(seqs)
    ask = SplitBuffers(0)
    st0 = ix.split_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), 0, 0, ask.starts.data_ptr(), 0, 0, solid_min, min_len, raise_on_capacity=False)
    nf, need = st0["n_fragments"], (st0["n_nts_out"] + 15) // 16 + 2
    assert (st0.pop("rc", 0) == ECAPACITY) == (nf > 0) and (nf > 0 or ask.host()[1][0] == 0)
    out = SplitBuffers(nf, need)
    st = ix.split_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), out.packed.data_ptr(), need, out.starts.data_ptr(), out.frags.data_ptr(), nf, solid_min, min_len)
    assert st == st0
    p, s, f = out.host()
    assert (p[need:] == FILL).all() and (s[nf + 1:] == np.uint64(2**64 - 1)).all() and (f[nf * 16:] == ROW_FILL).all()
    host_rows, host_st = ix.split_reads(seqs, solid_min, min_len)
    return p[:need].copy(), s[:nf + 1].copy(), out.rows(nf).copy(), st, host_rows, host_st


def batches(path, max_batch_reads):
    kw = dict(max_batch_reads=max_batch_reads) if max_batch_reads else {}
    out, checks = {}, 0
    for k, m, b in E2E_GEOMETRIES:
        seqs = error_reads(k, 300, seed=26)  # (few reads: with BRISK_PROFILE_BATCH=1 every read is a batch of every call)
        words, starts = device_reads(seqs)[2:]
        with brisk_amd.BriskHip(k, m, b, **kw) as ix:
            ix.insert_reads(seqs[:200])
            slots = ix.get_kmers(seqs)
            for solid_min, min_len in ((2, 0), (2, k + 20)):
                p, s, rows, st, host_rows, host_st = split_outputs(ix, seqs, solid_min, min_len)
                want, want_st = brisk_amd.fragments_from_slots(*slots, k, solid_min, min_len, n_nts_in=int(starts[-1]))
                assert np.array_equal(rows, want) and np.array_equal(host_rows, want) and st == want_st == host_st, (k, solid_min, min_len)
                want_p, want_s, _ = gather_reference(words, starts, want)
                assert np.array_equal(p, want_p) and np.array_equal(s, want_s)
                assert st["n_fragments"] > st["n_reads_kept"] > 5
                out[(k, solid_min, min_len)] = (p.tobytes(), s.tobytes(), rows.tobytes(), host_rows.tobytes(), sorted(st.items()), sorted(host_st.items()))
                checks += 1
    with open(path, "wb") as f:
        pickle.dump(out, f)
    return checks


def main():
    assert torch.cuda.is_available()
    if sys.argv[1] == "runs":
        print(f"ok {crafted_runs()}")
    else:
        print(f"ok {batches(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 0)}")


if __name__ == "__main__":
    main()
