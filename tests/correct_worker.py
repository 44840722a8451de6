"""Worker and shared helpers of test_correct.py.  As a program (one process per environment: the library reads BRISK_PROFILE_BATCH and
BRISK_CORRECT_BATCH once):
    correct_worker.py batches OUT.pkl [MAX]    correct_packed and correct_reads over error-bearing reads at both geometries (MAX:
                                               max_batch_reads of the handle); the bytes and the stats are left in OUT.pkl
prints "ok <n checks>"."""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # before the library: torch's HIP runtime first, as in the test process

import brisk_amd
from correct_reference import host_route
from extract_reference import pack_reads
from density_reads import as_strings, dense_reads
from extract_worker import E2E_GEOMETRIES, FILL, device_reads
from split_worker import ROW_FILL, SplitBuffers

ECAPACITY = 5


def route(ix, seqs, solid_min, min_cover):
    return host_route(ix, seqs, solid_min, min_cover, brisk_amd.sites_from_slots, brisk_amd.corrections_from_candidates)


def correct_outputs(ix, seqs, solid_min, min_cover, refusals=True):
    """correct_packed with exactly the room it needs (the stats asked for first, without outputs) and correct_reads:
    (words, rows, stats, host rows, host stats)"""
    d_packed, d_starts, words, starts = device_reads(seqs)
    st0 = ix.correct_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), 0, 0, 0, 0, solid_min, min_cover)
    nc, need = st0["n_corrected"], len(words)
    assert need == (int(starts[-1]) + 15) // 16 + 2
    out = SplitBuffers(nc, need)
    if nc and refusals:  # one row too few, one word too few: refused, the stats filled, nothing written
        for cap_words, corr_cap in ((need, nc - 1), (need - 1, nc)):
            st1 = ix.correct_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), out.packed.data_ptr(), cap_words, out.frags.data_ptr(), corr_cap, solid_min, min_cover,
                                    raise_on_capacity=False)
            assert st1.pop("rc") == ECAPACITY and st1 == st0 and out.untouched()
    st = ix.correct_packed(d_packed.data_ptr(), d_starts.data_ptr(), len(seqs), out.packed.data_ptr(), need, out.frags.data_ptr(), nc, solid_min, min_cover)
    assert st == st0
    p, s, f = out.host()
    assert (p[need:] == FILL).all() and (s == np.uint64(2**64 - 1)).all() and (f[nc * 16:] == ROW_FILL).all()
    host_rows, host_st = ix.correct_reads(seqs, solid_min, min_cover)
    return p[:need].copy(), f[:nc * 16].view(brisk_amd.CORRECTION_DTYPE).copy(), st, host_rows, host_st


def check_against_route(ix, seqs, solid_min, min_cover, refusals=True):
    """the composed calls against the host route: table, stats and output words equal; returns what the batch tests compare"""
    want, want_st, patched, _ = route(ix, seqs, solid_min, min_cover)
    p, rows, st, host_rows, host_st = correct_outputs(ix, seqs, solid_min, min_cover, refusals)
    assert st == want_st and host_st == want_st, (solid_min, min_cover, st, host_st, want_st)
    assert np.array_equal(rows, want) and np.array_equal(host_rows, want), (solid_min, min_cover)
    assert np.array_equal(p, pack_reads(patched)[0]), (solid_min, min_cover)
    assert st["n_runs"] == st["n_sites"] + st["n_skip_whole"] + st["n_skip_long"] + st["n_skip_short"]
    assert st["n_sites"] == st["n_corrected"] + st["n_ambiguous"] + st["n_unresolved"]
    return p, rows, st, host_rows, host_st


def batches(path, max_batch_reads):
    kw = dict(max_batch_reads=max_batch_reads) if max_batch_reads else {}
    out, checks = {}, 0
    for k, m, b in E2E_GEOMETRIES:
        # few reads (with BRISK_PROFILE_BATCH=1 every read is a batch of every call) over a small genome: dense enough for sites that are decided
        seqs = as_strings(*dense_reads(300, k, 2000, 27, e=0.01, n_special=40))
        with brisk_amd.BriskHip(k, m, b, **kw) as ix:
            ix.insert_reads(seqs[:200])
            for solid_min, min_cover in ((2, 0), (2, 1)):
                p, rows, st, host_rows, host_st = check_against_route(ix, seqs, solid_min, min_cover, refusals=False)
                print(k, solid_min, min_cover, st, file=sys.stderr)
                assert st["n_sites"] > 14 and st["n_corrected"] > 0  # more than two rounds at BRISK_CORRECT_BATCH=7
                out[(k, solid_min, min_cover)] = (p.tobytes(), rows.tobytes(), host_rows.tobytes(), sorted(st.items()), sorted(host_st.items()))
                checks += 1
    with open(path, "wb") as f:
        pickle.dump(out, f)
    return checks


def main():
    assert torch.cuda.is_available()
    print(f"ok {batches(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 0)}")


if __name__ == "__main__":
    main()
