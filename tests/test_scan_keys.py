"""The scan's order keys and its k > 32 re-scan on the device: the fast key of the body each geometry's scan runs against the exact
key, how many keys the exact fold decided, and index parity on reads built to expire.  The arithmetic itself is held on the host in
test_scan_keys_cpu.py."""
import random

import numpy as np
import pytest

import oracle
import scan_keys_inputs as SK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import brisk_amd
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return brisk_amd


# three geometries whose scan has k and m as compile-time constants, one with the run-time layout
@pytest.mark.parametrize("k,m,b", ((63, 21, 14), (31, 15, 14), (31, 11, 11), (47, 19, 12)))
def test_fast_key_is_exact_key(B, O, k, m, b):
    coef = O.coef_table(m)
    rng = random.Random(k * 100 + m)
    groups = {
        "random": [rng.getrandbits(2 * m) for _ in range(1 << 16)],
        "periodic": SK.periodic_mmers(m),
        "padded": SK.padded_mmers(m, rng),
        "near_eps": [int(x) for x in SK.near_eps_mmers(m, coef, seed=m)],
        "band": [int(x) for x in SK.band_mmers(m, coef, seed=5)],  # m-mers put together to lie in the band: only m = 19 has any
    }
    guards = {}
    with B.BriskHip(k, m, b, part_bits=2) as ix:
        for name, xs in groups.items():
            if not xs:
                guards[name] = 0
                continue
            fast = ix.debug_order_keys(xs)
            guards[name] = ix.debug_guard_count()
            exact = ix.debug_order_keys(xs, exact=True)
            assert ix.debug_guard_count() == 0
            assert np.array_equal(fast, exact), name
            if name != "random":
                assert np.array_equal(fast, O.key_many(xs, m)), name
            # the guard path is taken by exactly the keys whose integer sums lie in the band (the tables restated on the host)
            want = int(SK.decode_biased(*SK.table_sums(np.array(xs, np.uint64), m, coef))[1].sum())
            print(f"k={k} m={m} {name}: {len(xs)} keys, {guards[name]} through the exact fold (host restatement: {want})")
            assert guards[name] == want, name
    assert guards["periodic"] == 0
    # the fold is exercised: by the m-mers nearest to +-eps where the sample holds one inside the band, else by the ones put together
    # for it (m = 11, 15 and 21 have no m-mer inside the band at all -- test_scan_keys_cpu.py holds that by exhaustive search --: nothing can exercise it there)
    if m == 19:
        assert guards["near_eps"] + guards["band"] >= 1


def _parity(B, O, reads, k, m, b):
    want = O.count(reads, k, m, b)
    with B.BriskHip(k, m, b) as ix:
        ix.insert_reads(reads)
        st = ix.stats()
        got = oracle.multiset_lines(*ix.enumerate(), k)
    assert (st["nb_kmers"], st["nb_buckets"]) == want[1:]
    assert got == want[0]


@pytest.mark.parametrize("k,m,b", ((63, 21, 14), (47, 19, 12)))
def test_rescan_parity_long_k(B, O, k, m, b):
    """k > 32: the re-scan rounds on homopolymers, period-2 and period-3 stretches, and zero-padded windows that tie with each other
    and with the all-A m-mer."""
    _parity(B, O, SK.rescan_reads(k * 100 + m), k, m, b)


def test_rescan_parity_short_k_unchanged(B, O):
    """k = 31, m = 15: the window minimum comes from the lanes' queues and the re-scan from whole k-mers"""
    _parity(B, O, SK.rescan_reads(3115), 31, 15, 14)
