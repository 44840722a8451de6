"""Worker and shared helpers of test_extract.py.  As a program (one process per environment: the library reads BRISK_PROFILE_SEG
once): the end-to-end case -- trim on the device and recount, against the host route -- at both geometries; prints "ok <n checks>"."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # before the library: torch's HIP runtime first, as in the test process

import brisk_amd
from density_reads import as_strings, dense_reads
from extract_reference import pack_reads

E2E_GEOMETRIES = ((63, 21, 14), (31, 11, 11))
FILL = 0x5AA5C33C  # what an output buffer holds before a call


def error_reads(k, n=3000, seed=7):
    """error-bearing reads at ~20x over a small genome (lengths 100 / 150 / 250, a ragged tail around k, 1 % substitutions, N cuts,
    some lower case): most k-mers are seen many times, the ones that carry an error once"""
    flat, offs = dense_reads(n, k, 24_000, seed, e=0.01, n_special=40)
    return as_strings(flat, offs)


def device_reads(seqs):
    """(d_packed, d_starts, words, starts): the stream with its two readable words, on the device and on the host"""
    words, starts = pack_reads(seqs)
    d_packed = torch.from_numpy(words.view(np.int32)).cuda()
    d_starts = torch.from_numpy(starts.view(np.int64)).cuda()
    return d_packed, d_starts, words, starts


class OutBuffers:
    """output buffers of one extract / trim call, pre-filled: cap words and four more that no call may touch"""

    def __init__(self, n_reads, cap):
        self.cap = cap
        self.packed = torch.full((cap + 4,), FILL, dtype=torch.int32, device="cuda")
        self.starts = torch.full((n_reads + 2,), -1, dtype=torch.int64, device="cuda")
        self.index = torch.full((max(n_reads, 1) + 1,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def host(self):
        torch.cuda.synchronize()
        return self.packed.cpu().numpy().view(np.uint32), self.starts.cpu().numpy().view(np.uint64), self.index.cpu().numpy().view(np.uint64)

    def untouched(self):
        p, s, i = self.host()
        return (p == FILL).all() and (s == np.uint64(0xffffffffffffffff)).all() and (i == np.uint64(0xffffffffffffffff)).all()


def host_route(ix, seqs, solid_min, rule):
    """get_kmers -> profile_from_slots -> intervals_from_profile -> Python slicing: (intervals, [(read index, kept string)])"""
    ivs = brisk_amd.intervals_from_profile(brisk_amd.profile_from_slots(*ix.get_kmers(seqs), solid_min), ix.k, rule)
    return ivs, [(i, s[int(v["start"]):int(v["start"]) + int(v["len"])]) for i, (s, v) in enumerate(zip(seqs, ivs)) if v["len"]]


def end_to_end(k, m, b, **kw):
    """index A from error-bearing reads; B counts what trim_packed keeps of them, C what the host route keeps: the same index"""
    seqs = error_reads(k)
    rule = brisk_amd.select_rule("solid_run")
    with brisk_amd.BriskHip(k, m, b, **kw) as A, brisk_amd.BriskHip(k, m, b) as B, brisk_amd.BriskHip(k, m, b) as C:
        A.insert_reads(seqs)
        d_packed, d_starts, words, _ = device_reads(seqs)
        out = OutBuffers(len(seqs), len(words))
        n_out, n_nts = A.trim_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), out.packed.data_ptr(), out.cap, out.starts.data_ptr(), out.index.data_ptr(), 2, rule)
        B.insert_packed(out.packed.data_ptr(), out.starts.data_ptr(), n_out)
        _, kept = host_route(A, seqs, 2, rule)
        C.insert_reads([s for _, s in kept])
        got, want = B.checksum(), C.checksum()
        _, o_starts, o_index = out.host()
    assert 0 < n_out < len(seqs), (n_out, len(seqs))
    assert (n_out, n_nts) == (len(kept), sum(len(s) for _, s in kept)), (k, kw, n_out, n_nts, len(kept))
    assert o_index[:n_out].tolist() == [i for i, _ in kept]
    assert int(o_starts[n_out]) == n_nts
    assert any(len(s) < len(seqs[i]) for i, s in kept), "no read was trimmed: the reads carry no errors?"
    assert got == want and got[0] > 0, (k, kw, got, want)


def main():
    assert torch.cuda.is_available()
    checks = 0
    for k, m, b in E2E_GEOMETRIES:
        end_to_end(k, m, b)
        checks += 1
    print(f"ok {checks}")


if __name__ == "__main__":
    main()
