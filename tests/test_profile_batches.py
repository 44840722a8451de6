"""GPU: the internal batches of the read-cleaning calls.  read_profile / trim / trim_pairs / clean_pairs, host and packed, walk their
reads in batches of min(max_batch_reads, BRISK_PROFILE_BATCH) reads; the library reads that setting (and BRISK_PROFILE_SEG) once per
process, so every environment is a child: profile_batches_worker.py checks each call against the numpy definitions and the refusals
whose fault lies in a later batch, and leaves its outputs behind.  Here: every environment passes, and the outputs are the same
bytes whatever the batches are -- one read a batch, five (a batch ends between the mates of the third pair; the read of three
segments lies in the second batch), or the whole call in one."""
import os
import pickle
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "profile_batches_worker.py")
ENVIRONMENTS = {"batch1": dict(BRISK_PROFILE_BATCH="1"), "batch5": dict(BRISK_PROFILE_BATCH="5"), "whole": {}, "batch5_seg64": dict(BRISK_PROFILE_BATCH="5", BRISK_PROFILE_SEG="64")}
_outputs = {}


def outputs_of(name, tmp_path_factory):
    """the worker's outputs in that environment: run once, shared by the tests"""
    if name not in _outputs:
        env = {k: v for k, v in os.environ.items() if k not in ("BRISK_PROFILE_BATCH", "BRISK_PROFILE_SEG")}
        env.update(ENVIRONMENTS[name])
        path = str(tmp_path_factory.mktemp("batches") / (name + ".pkl"))
        p = subprocess.run([sys.executable, WORKER, path], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and p.stdout.strip().endswith("ok 32"), (name, p.stdout[-2000:], p.stderr[-4000:])
        with open(path, "rb") as f:
            _outputs[name] = pickle.load(f)
    return _outputs[name]


@pytest.mark.parametrize("name", list(ENVIRONMENTS))
def test_every_call_against_the_numpy_definitions(name, tmp_path_factory):
    out = outputs_of(name, tmp_path_factory)
    assert len(out) > 60 and all(len(v) for k, v in out.items() if k.endswith(("intervals", "counts")) or k.startswith("profile"))


def test_outputs_do_not_depend_on_the_batches(tmp_path_factory):
    whole = outputs_of("whole", tmp_path_factory)
    for name in ("batch1", "batch5", "batch5_seg64"):
        got = outputs_of(name, tmp_path_factory)
        assert sorted(got) == sorted(whole), name
        assert [k for k in whole if got[k] != whole[k]] == [], name
