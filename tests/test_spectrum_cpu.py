"""No GPU: the abundance entry points (count spectrum, count-range enumeration, prune) are declared in the header, listed in
hipapi.SYMBOLS, exported by the built library, and wrapped with the documented default arguments."""
import inspect
import os
import re

import pytest

import brisk_amd
from brisk_amd import hipapi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("brisk_hip_count_spectrum", "brisk_hip_enumerate_range", "brisk_hip_prune")


@pytest.fixture(scope="module")
def lib():
    brisk_amd.build_library()
    return hipapi.load()


def test_names_are_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(brisk_hip_[a-z_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared, name
        assert name in hipapi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.brisk_hip_abi_version() == 4  # additive change


def test_wrappers_and_their_defaults():
    sig = inspect.signature(brisk_amd.BriskHip.enumerate)
    assert sig.parameters["min_count"].default == 0 and sig.parameters["max_count"].default == 255
    assert list(sig.parameters)[:2] == ["self", "chunk"]  # today's positional call keeps its meaning
    sig = inspect.signature(brisk_amd.BriskHip.prune)
    assert list(sig.parameters) == ["self", "min_count", "max_count"]
    assert sig.parameters["min_count"].default is inspect.Parameter.empty and sig.parameters["max_count"].default == 255
    assert list(inspect.signature(brisk_amd.BriskHip.count_spectrum).parameters) == ["self"]


def test_null_handle_is_refused_without_a_device(lib):
    import ctypes as C
    import numpy as np
    out = np.zeros(256, np.uint64)
    assert lib.brisk_hip_count_spectrum(None, out) == 1  # EINVAL
    assert lib.brisk_hip_prune(None, 1, 255, None) == 1
    cur, n = C.c_uint64(0), C.c_uint64(0)
    a, b = np.zeros(1, np.uint64), np.zeros(1, np.uint8)
    assert lib.brisk_hip_enumerate_range(None, C.byref(cur), a, a, b, b, 1, C.byref(n), 0, 255) == 1


def test_kff_writer_and_counter_know_the_bounds():
    kff = open(os.path.join(ROOT, "brisk_amd", "include", "brisk_kff.hpp")).read()
    assert re.search(r"brisk_write_kff\([^)]*uint32_t min_count = 0, uint32_t max_count = 255\)", kff)
    app = open(os.path.join(ROOT, "brisk_amd", "apps", "brisk_count.cpp")).read()
    for opt in ("--histo", "--min-count", "--max-count"):
        assert opt in app
