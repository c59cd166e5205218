"""The host-only generator of the TDT's family flips (include/hpgv.h hpgv_perm_flips_shuffle) against a Python re-statement of
it.  No device: it is a plain function of libhpgv.so."""
import ctypes as C

import numpy as np
import pytest

from helpers import hpgv

M64 = (1 << 64) - 1


def _mix(z):
    """SplitMix64 as include/hpgv.h states it"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _flips(n_families, n_perms, seed):
    out = np.zeros((n_perms, n_families), np.uint8)
    for p in range(n_perms):
        key = _mix((seed ^ _mix(p)) & M64)
        for f in range(n_families):
            out[p, f] = (_mix((key + (f >> 6)) & M64) >> (f & 63)) & 1
    return out


@pytest.mark.parametrize("n_perms", [0, 1, 17])
@pytest.mark.parametrize("n_families", [0, 1, 63, 64, 65, 200])
def test_generator_bit_for_bit(n_families, n_perms):
    for seed in (0, 20240611, M64):
        got = hpgv.perm_flips_shuffle(n_families, n_perms, seed)
        assert got.shape == (n_perms, n_families) and got.dtype == np.uint8
        assert np.array_equal(got, _flips(n_families, n_perms, seed))


def test_two_seeds_differ_and_a_row_depends_on_its_index_alone():
    a, b = hpgv.perm_flips_shuffle(200, 17, 1), hpgv.perm_flips_shuffle(200, 17, 2)
    assert (a != b).any(axis=1).all()                     # 200 fair bits per row: equal rows do not happen
    assert np.array_equal(hpgv.perm_flips_shuffle(200, 5, 1), a[:5])
    assert len({r.tobytes() for r in a}) == 17


def test_every_row_holds_both_values():
    a = hpgv.perm_flips_shuffle(200, 17, 99)
    assert set(np.unique(a)) == {0, 1}
    assert ((a == 0).any(axis=1) & (a == 1).any(axis=1)).all()
    # a fair coin: the share of ones over 3 400 draws lies within five standard deviations of a half
    assert abs(a.mean() - 0.5) <= 5 * 0.5 / np.sqrt(a.size)


def test_argument_errors():
    L = hpgv.load()
    buf = np.zeros(64, np.uint8)
    ptr = C.c_void_p(buf.ctypes.data)
    assert L.hpgv_perm_flips_shuffle(-1, 1, 0, ptr) == hpgv.ERR_INVALID
    assert L.hpgv_perm_flips_shuffle(1, -1, 0, ptr) == hpgv.ERR_INVALID
    assert L.hpgv_perm_flips_shuffle(4, 4, 0, None) == hpgv.ERR_INVALID
    assert L.hpgv_perm_flips_shuffle(0, 4, 0, None) == hpgv.OK        # nothing to write
    assert L.hpgv_perm_flips_shuffle(4, 0, 0, None) == hpgv.OK
