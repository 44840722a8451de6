"""CPU-side checks of the joint count spectrum and the joint count-window filter: the boundary (header, symbol table, wrapper
signatures), the refusals that return before any device is touched, the two host-only functions (joint_spectrum_from_entries,
joint_figures) against hand-made cases, and the app's options.  What the kernels compute is tests/test_joint.py (GPU)."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import brisk_amd
from brisk_amd import hipapi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["brisk_hip_joint_spectrum", "brisk_hip_filter_joint"]
EINVAL = 1
A = 256  # the absent state


@pytest.fixture(scope="module")
def lib():
    brisk_amd.build_library()
    return hipapi.load()


def header():
    return open(os.path.join(ROOT, "include", "brisk_hip.h")).read()


def dump(rows):
    """(lo, hi, minimizer_idx, count) arrays, as enumerate returns them, from (hi, lo, idx, count) rows"""
    return (np.array([r[1] for r in rows], np.uint64), np.array([r[0] for r in rows], np.uint64), np.array([r[2] for r in rows], np.uint8),
            np.array([r[3] for r in rows], np.uint8))


def matrix(bins):
    J = np.zeros((257, 257), np.uint64)
    for (sa, sb), n in bins.items():
        J[sa, sb] = n
    return J


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def test_declared_listed_and_exported(lib):
    hdr = header()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared, name
        assert name in hipapi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.brisk_hip_abi_version() == 4  # additions only
    assert re.search(r"#define\s+BRISK_HIP_ABI_VERSION\s+4\b", hdr)
    assert re.search(r"#define\s+BRISK_HIP_JOINT_ABSENT\s+256u\b", hdr) and re.search(r"#define\s+BRISK_HIP_JOINT_STATES\s+257u\b", hdr)
    assert brisk_amd.JOINT_ABSENT == 256


def test_the_window_struct_is_the_headers():
    body = re.search(r"typedef struct brisk_hip_joint_window \{(.*?)\} brisk_hip_joint_window;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in re.findall(r"uint32_t\s+([^;]+);", body) for n in decl.split(",")]
    assert fields == ["min_self", "max_self", "min_other", "max_other", "keep_absent", "reserved"]
    assert [n for n, _ in hipapi._JointWindow._fields_] == fields and C.sizeof(hipapi._JointWindow) == 24


def test_wrapper_signatures():
    H = brisk_amd.BriskHip
    assert list(inspect.signature(H.joint_spectrum).parameters) == ["self", "other"]
    sig = inspect.signature(H.filter_joint)
    assert list(sig.parameters) == ["self", "other", "min_self", "max_self", "min_other", "max_other", "keep_absent"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [0, 255, 0, 255, False]
    assert list(inspect.signature(brisk_amd.joint_spectrum_from_entries).parameters) == ["dump_a", "dump_b"]
    sig = inspect.signature(brisk_amd.joint_figures)
    assert list(sig.parameters) == ["joint", "k", "solid_min"] and sig.parameters["solid_min"].default == 2


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_null_arguments_are_einval_without_a_device(lib):
    out = np.zeros(257 * 257, np.uint64)
    n = C.c_uint64(7)
    w = hipapi._JointWindow(0, 255, 0, 255, 0, 0)
    fake = C.c_void_p(8)  # never dereferenced: the null first handle is refused before anything else is looked at
    assert lib.brisk_hip_joint_spectrum(None, None, out.ctypes.data) == EINVAL
    assert lib.brisk_hip_joint_spectrum(None, fake, out.ctypes.data) == EINVAL
    assert lib.brisk_hip_joint_spectrum(None, None, None) == EINVAL
    assert lib.brisk_hip_filter_joint(None, None, C.byref(w), C.byref(n)) == EINVAL
    assert lib.brisk_hip_filter_joint(None, fake, C.byref(w), C.byref(n)) == EINVAL
    assert lib.brisk_hip_filter_joint(None, None, None, C.byref(n)) == EINVAL
    assert lib.brisk_hip_filter_joint(None, None, None, None) == EINVAL
    assert n.value == 7 and not out.any()  # nothing written


def test_a_bad_bound_is_a_value_error_before_any_call():
    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    ix = object.__new__(brisk_amd.BriskHip)  # no handle, no device
    ix.L, ix.h = NoLibrary(), C.c_void_p()
    for bad in (dict(min_self=-1), dict(max_self=2.5), dict(min_other="3"), dict(max_other=None), dict(min_self=True), dict(min_self=9, max_self=8),
                dict(min_other=1, max_other=0), dict(min_other=7, max_other=3, keep_absent=False)):
        with pytest.raises(ValueError):
            ix.filter_joint(ix, **bad)
    with pytest.raises(AssertionError, match="brisk_hip_filter_joint"):  # a good window does reach the library
        ix.filter_joint(ix, min_other=1, max_other=0, keep_absent=True)


# ---- joint_spectrum_from_entries on hand-made dumps ------------------------------------------------------------------------------------
def test_from_entries_hand_made():
    # (hi, lo, idx, count).  shared with counts (0, 255); only in a with count 0; only in b; one k-mer under two minimizer positions
    a = dump([(0, 5, 3, 0), (0, 6, 3, 0), (1, 9, 2, 7), (1, 9, 4, 8)])
    b = dump([(1, 9, 4, 2), (0, 5, 3, 255), (2, 5, 3, 9), (1, 9, 5, 1)])
    J = brisk_amd.joint_spectrum_from_entries(a, b)
    assert J.shape == (257, 257) and J.dtype == np.uint64
    want = {(0, 255): 1,  # (0, 5, 3): a wrapped count of 0 is present
            (0, A): 1,    # (0, 6, 3): only in a, state 0 -- not "absent"
            (7, A): 1,    # (1, 9, 2): the same k-mer as (1, 9, 4) and (1, 9, 5), another identity
            (8, 2): 1,    # (1, 9, 4)
            (A, 9): 1,    # (2, 5, 3): lo and idx of a shared entry, another hi
            (A, 1): 1}    # (1, 9, 5)
    assert np.array_equal(J, matrix(want))
    assert np.array_equal(brisk_amd.joint_spectrum_from_entries(b, a), matrix(want).T)
    assert J[A, A] == 0


def test_from_entries_empty_dumps():
    empty = dump([])
    one = dump([(0, 1, 2, 3)])
    assert not brisk_amd.joint_spectrum_from_entries(empty, empty).any()
    assert np.array_equal(brisk_amd.joint_spectrum_from_entries(one, empty), matrix({(3, A): 1}))
    assert np.array_equal(brisk_amd.joint_spectrum_from_entries(empty, one), matrix({(A, 3): 1}))
    assert np.array_equal(brisk_amd.joint_spectrum_from_entries(one, one), matrix({(3, 3): 1}))


# ---- joint_figures against closed forms ------------------------------------------------------------------------------------------------
def test_figures_of_a_diagonal_matrix():
    f = brisk_amd.joint_figures(matrix({(1, 1): 50, (2, 2): 30, (40, 40): 5}), k=31)
    assert (f["shared"], f["only_self"], f["only_other"]) == (85, 0, 0)
    assert f["error_rate"] == 0 and f["qv"] == math.inf and f["completeness"] == 1.0
    assert tuple(f) == ("shared", "only_self", "only_other", "completeness", "error_rate", "qv")


def test_figures_error_rate_closed_form():
    # only_self / entries = 1 - 0.999**k  <=>  error_rate = 0.001.  k = 21: 1 - 0.999**21 = 0.020791...; 10^6 entries
    k = 21
    entries = 10 ** 6
    only_self = round(entries * (1 - 0.999 ** k))
    f = brisk_amd.joint_figures(matrix({(1, 30): entries - only_self, (1, A): only_self, (A, 1): 12345}), k=k)
    assert (f["shared"], f["only_self"], f["only_other"]) == (entries - only_self, only_self, 12345)
    assert abs(f["error_rate"] - 0.001) < 1e-7  # (rounding only_self to an integer moves the share by < 1e-6, the rate by < 1e-6 / k)
    assert abs(f["qv"] - 30.0) < 1e-3


def test_figures_completeness_and_solid_min():
    # other's entries: count 1: 10 shared, 90 not; count 2: 40 shared, 10 not; count 3: 45 shared, 5 not
    J = matrix({(1, 1): 10, (A, 1): 90, (1, 2): 40, (A, 2): 10, (5, 3): 45, (A, 3): 5, (1, A): 3})
    assert brisk_amd.joint_figures(J, 31)["completeness"] == 85 / 100  # the default: solid_min = 2
    assert brisk_amd.joint_figures(J, 31, solid_min=1)["completeness"] == 95 / 200  # bin 1 moves in
    assert brisk_amd.joint_figures(J, 31, solid_min=3)["completeness"] == 45 / 50  # bin 2 moves out
    assert math.isnan(brisk_amd.joint_figures(J, 31, solid_min=4)["completeness"])  # no solid entry at all
    with pytest.raises(ValueError):
        brisk_amd.joint_figures(np.zeros((256, 256), np.uint64), 31)
    assert "distinct" in brisk_amd.joint_figures.__doc__.lower()


# ---- the app, the oracle ---------------------------------------------------------------------------------------------------------------
def test_brisk_count_knows_the_options():
    src = open(os.path.join(ROOT, "brisk_amd", "apps", "brisk_count.cpp")).read()
    for opt in ("--joint", "--joint-histo", "--filter-joint", "--window"):
        assert '"%s"' % opt in src, opt
    assert "brisk_hip_joint_spectrum(" in src and "brisk_hip_filter_joint(" in src


def test_the_product_still_never_touches_the_oracle():
    from test_capi_cpu import test_product_never_touches_the_oracle
    test_product_never_touches_the_oracle()
