"""GPU: random sequences of the public operations over two handles, checked against a host model after every operation.

The model, the generator and the committed seeds are tests/index_model.py (checked without a device by
tests/test_index_model_cpu.py); the replay and its checks are tests/op_sequence_worker.py.  After EVERY operation: its return
value, checksum, nb_kmers, nb_buckets, count_spectrum and the whole enumeration of the handle that changed, the same of `other`
after a two-index operation, and a lookup of 2 000 fixed identities.  After every eighth and at the end: a count-range
enumeration, compare, joint_spectrum and get_kmers over 60 reads.  A failure names the seed, the operation and the operations so
far; `python tests/op_sequence_worker.py SEED GEOMETRY MODE` replays it."""
import os
import subprocess
import sys

import pytest

from index_model import GEOMETRIES, MODES, SEEDS, make_case

pytestmark = pytest.mark.gpu

CASES = [(g, mode, seed) for g in GEOMETRIES for mode in MODES for seed in SEEDS[g, mode]]
VARIANTS = [{"BRISK_INSERT_GENERIC": "1", "BRISK_QUERY_GENERIC": "1"}, {"BRISK_BINS": "0"}, {"BRISK_HUGE_AT": "64", "BRISK_HUGE_QUERY_AT": "64"}, {"BRISK_DEFER": "0"}]


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


@pytest.mark.parametrize("geometry,mode,seed", CASES, ids=["%s-%s-%d" % c for c in CASES])
def test_sequence_matches_the_model(B, O, tmp_path, geometry, mode, seed):
    from op_sequence_worker import replay
    seconds = replay(B, O, make_case(seed, geometry, mode), str(tmp_path))
    print("%s %s seed %d: %.1f s" % (geometry, mode, seed, seconds))


@pytest.mark.parametrize("extra", VARIANTS, ids=["+".join("%s=%s" % kv for kv in v.items()) for v in VARIANTS])
def test_sequences_under_kernel_variants(extra):
    """the bodies and layouts the default settings do not reach by themselves: one fresh process per setting, nothing retried"""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "op_sequence_worker.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("BRISK_") or k == "BRISK_HIP_LIB"}
    p = subprocess.run([sys.executable, worker], env=dict(env, **extra), capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok 3"), (extra, p.stdout[-3000:], p.stderr[-6000:])
