"""hpgv_clump (include/hpgv.h): the clump assignment against a direct Python loop.  Host only: no device, no context."""
import numpy as np
import pytest

from clump_golden import clump_loop as loop
from helpers import hpgv


def check(p, pairs, p1):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    got = hpgv.clump(p, pairs, p1)
    exp = loop(list(map(float, p)), pairs.tolist(), p1)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    return got


@pytest.mark.parametrize("n", [0, 1, 2, 50, 400])
def test_random_graphs(n):
    rng = np.random.default_rng(40 + n)
    for density in (0.0, 1.5, 6.0):
        m = int(n * density) if n > 1 else 0
        pairs = rng.integers(0, max(n, 1), (m, 2))
        p = rng.random(n) * 2e-3
        index_of, order = check(p, pairs, 1e-3)
        if n >= 50:
            assert 0 < len(order) < n
        # every claimed candidate names an index that names itself
        claimed = index_of >= 0
        assert (index_of[index_of[claimed]] == index_of[claimed]).all()
    if n >= 50:
        # the records of an edge list (hpgv_ld_edge) and plain pairs are the same input
        e = np.zeros(len(pairs), hpgv.LD_EDGE)
        e["a"], e["b"], e["r2"] = pairs[:, 0], pairs[:, 1], 0.7
        a, b = hpgv.clump(p, e, 1e-3), hpgv.clump(p, pairs, 1e-3)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_ties_go_to_the_lower_number():
    p = np.array([0.5, 1e-5, 1e-5, 1e-5, 1e-6])
    index_of, order = check(p, [(1, 2), (3, 2)], 1e-4)
    assert order.tolist() == [4, 1, 3] and index_of.tolist() == [-1, 1, 1, 3, 4]
    index_of, order = check(p, [(2, 1), (2, 3), (0, 3)], 1e-4)
    assert order.tolist() == [4, 1, 3] and index_of.tolist() == [3, 1, 1, 3, 4]


def test_p_equal_to_p1_is_an_index():
    p = np.array([1e-4, np.nextafter(1e-4, 1.0), np.nextafter(1e-4, 0.0)])
    index_of, order = check(p, [], 1e-4)
    assert order.tolist() == [2, 0] and index_of.tolist() == [0, -1, 2]


def test_chain_with_rising_p():
    # a - b - c: b is claimed by a, so c is an index of its own and does not get b
    index_of, order = check(np.array([1e-8, 1e-7, 1e-6]), [(0, 1), (1, 2)], 1e-4)
    assert order.tolist() == [0, 2] and index_of.tolist() == [0, 0, 2]
    # with c above p1 nobody claims it
    index_of, order = check(np.array([1e-8, 1e-7, 1e-3]), [(0, 1), (1, 2)], 1e-4)
    assert order.tolist() == [0] and index_of.tolist() == [0, 0, -1]


def test_nan_p():
    p = np.array([np.nan, 1e-6, np.nan, 1e-5])
    index_of, order = check(p, [(0, 1), (2, 3), (0, 2)], 1e-4)
    # a NaN candidate is no index, but may be claimed
    assert order.tolist() == [1, 3] and index_of.tolist() == [1, 1, 3, 3]
    index_of, order = check(np.array([np.nan, np.nan]), [(0, 1)], 1.0)
    assert len(order) == 0 and index_of.tolist() == [-1, -1]


def test_duplicate_reversed_and_self_edges():
    p = np.array([1e-6, 1e-5, 1e-5, 0.3])
    once = check(p, [(0, 3), (1, 2)], 1e-4)
    many = check(p, [(0, 3), (3, 0), (0, 3), (2, 1), (1, 2), (1, 1), (3, 3)], 1e-4)
    assert np.array_equal(once[0], many[0]) and np.array_equal(once[1], many[1])
    assert once[0].tolist() == [0, 1, 1, 0]


def test_refusals():
    p = np.array([1e-6, 1e-5])
    for bad in ([(0, 2)], [(-1, 1)], [(0, 1), (5, 0)]):
        with pytest.raises(hpgv.HpgvError) as err:
            hpgv.clump(p, bad, 1e-4)
        assert err.value.code == hpgv.ERR_INVALID
    with pytest.raises(hpgv.HpgvError):
        hpgv.clump(np.zeros(0), [(0, 0)], 1e-4)              # no candidate at all: every endpoint is outside
    L = hpgv.load()
    assert L.hpgv_clump(2, hpgv._ptr(p), None, 0, 1e-4, None, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_clump(-1, hpgv._ptr(p), None, 0, 1e-4, None, None, None) == hpgv.ERR_INVALID


def test_clump_order_may_be_null():
    import ctypes as C
    p = np.array([1e-6, 1e-5, 0.5])
    index_of = np.zeros(3, np.int32)
    k = C.c_int(-1)
    assert hpgv.load().hpgv_clump(3, hpgv._ptr(p), None, 0, 1e-4, hpgv._ptr(index_of), None, C.byref(k)) == hpgv.OK
    assert k.value == 2 and index_of.tolist() == [0, 1, -1]
