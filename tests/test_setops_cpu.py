"""CPU-side checks of the set operations (merge, intersect, subtract, compare): the boundary only -- header, symbol table,
wrapper signatures, argument refusals that return before any device is touched, and the app's options.  What the kernels
compute is tests/test_setops.py (GPU)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import brisk_amd
from brisk_amd import hipapi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["brisk_hip_merge", "brisk_hip_intersect", "brisk_hip_subtract", "brisk_hip_compare"]
EINVAL = 1


@pytest.fixture(scope="module")
def lib():
    brisk_amd.build_library()
    return hipapi.load()


def header():
    return open(os.path.join(ROOT, "include", "brisk_hip.h")).read()


def test_declared_listed_and_exported(lib):
    declared = set(re.findall(r"\b(brisk_hip_[a-z_]+)\s*\(", header()))
    for name in NAMES:
        assert name in declared, name
        assert name in hipapi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.brisk_hip_abi_version() == 4  # additions only
    assert re.search(r"#define\s+BRISK_HIP_ABI_VERSION\s+4\b", header())


def test_count_rule_constants():
    hdr = header()
    for name, value in (("LEFT", 0), ("MIN", 1), ("MAX", 2), ("SUM", 3)):
        assert re.search(r"\bBRISK_HIP_COUNT_%s\s*=\s*%d\b" % (name, value), hdr), name
    assert brisk_amd.BriskHip.COUNT_RULES == {"left": 0, "min": 1, "max": 2, "sum": 3}


def test_wrapper_signatures():
    H = brisk_amd.BriskHip
    assert list(inspect.signature(H.merge).parameters) == ["self", "other"]
    assert list(inspect.signature(H.subtract).parameters) == ["self", "other"]
    assert list(inspect.signature(H.compare).parameters) == ["self", "other"]
    sig = inspect.signature(H.intersect)
    assert list(sig.parameters) == ["self", "other", "count"] and sig.parameters["count"].default == "left"


def test_a_wrong_count_is_a_value_error_before_any_call():
    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    ix = object.__new__(brisk_amd.BriskHip)  # no handle, no device
    ix.L, ix.h = NoLibrary(), C.c_void_p()
    for bad in ("MIN", "first", "", None, 1):
        with pytest.raises(ValueError):
            ix.intersect(ix, count=bad)


def test_null_handles_are_einval_without_a_device(lib):
    out = np.zeros(6, np.uint64)
    n = C.c_uint64(7)
    assert lib.brisk_hip_merge(None, None, C.byref(n)) == EINVAL
    assert lib.brisk_hip_intersect(None, None, 0, C.byref(n)) == EINVAL
    assert lib.brisk_hip_subtract(None, None, C.byref(n)) == EINVAL
    assert lib.brisk_hip_compare(None, None, out) == EINVAL
    assert lib.brisk_hip_merge(None, None, None) == EINVAL  # the counter may be NULL as well
    assert n.value == 7 and not out.any()  # nothing written


def test_brisk_count_knows_the_options():
    src = open(os.path.join(ROOT, "brisk_amd", "apps", "brisk_count.cpp")).read()
    for opt, call in (("--merge", "brisk_hip_merge"), ("--subtract", "brisk_hip_subtract"), ("--intersect", "brisk_hip_intersect")):
        assert '"%s"' % opt in src and call + "(" in src, opt


def test_the_product_still_never_touches_the_oracle():
    from test_capi_cpu import test_product_never_touches_the_oracle
    test_product_never_touches_the_oracle()
    assert os.path.exists(os.path.join(ROOT, "brisk_amd", "csrc", "brisk_setops.hip"))  # and the walk saw the new file
