"""The row-range plan that the kernels over sample columns share (cols_plan_rows, csrc/hpgv_cols_kernels.h) without a device: the
three exports against the three formulas they replaced, written out here a second time.  This copy is the reference."""
import numpy as np
import pytest

from helpers import hpgv


@pytest.fixture(scope="module", autouse=True)
def built():
    hpgv.build()


def _up(a, b):
    return -(-a // b)


def _grm_rows(nv, nc, cus):
    """grm_plan_rows as it stood: four workgroups per CU deep over the tile pairs, ranges of at most 32 768 rows"""
    nv = max(nv, 0)
    tiles = _up(max(nc, 1), 64)
    pairs = tiles * (tiles + 1) // 2
    want, room = _up(4 * max(cus, 1), pairs), _up(nv, 256)
    splits = max(want, 1) if want < room else max(room, 1)
    splits = max(splits, _up(nv, 32768))
    return max(_up(_up(nv, splits), 64) * 64, 64)


def _score_rows(nv, nc, cus):
    """score_plan_rows as it stood: eight workgroups per CU deep over the tiles, ranges of at most 2^22 rows"""
    nv = max(nv, 0)
    tiles = _up(max(nc, 1), 64)
    want, room = _up(8 * max(cus, 1), tiles), _up(nv, 256)
    splits = max(want, 1) if want < room else max(room, 1)
    splits = max(splits, _up(nv, 1 << 22))
    return max(_up(_up(nv, splits), 64) * 64, 64)


def _ibs_rows(nv, nc, cus):
    """the arithmetic that stood inline in k_ibs_pairs's launch, which ran from one row and two columns on a device with at least one
    CU.  Outside that it divides by zero (no column) or yields no rows (no row); there this copy takes grm_plan_rows's guards -- a
    column count and a CU count of at least 1, at least 64 rows -- which change nothing inside."""
    tiles = _up(max(nc, 1), 64)
    pairs = tiles * (tiles + 1) // 2
    want, room = _up(4 * max(cus, 1), pairs), _up(nv, 256)
    splits = max(1, min(want, room))
    return max(_up(_up(nv, splits), 64) * 64, 64)


def _shapes():
    """the shapes of test_grm_cpu.test_no_row_range_overflows_an_i32_sum, and 300 random ones"""
    shapes = [(10 ** 6, 3000, 256), (70000, 20, 256), (2 ** 31 - 1, 1, 256), (2 ** 31 - 1, 100000, 256), (2 ** 31 - 1, 3000, 1), (0, 0, 0), (1, 1, 1),
              (32769, 3000, 256), (65536, 5000, 304), (66053, 2048, 64)]
    rng = np.random.default_rng(4)
    shapes += [(int(10 ** rng.uniform(0, 9.3)), int(10 ** rng.uniform(0, 5)), int(rng.integers(1, 400))) for _ in range(300)]
    return shapes


def test_grm_and_score_plans_are_the_formulas_they_were():
    for nv, nc, cus in _shapes():
        assert hpgv.grm_plan_rows(nv, nc, cus) == _grm_rows(nv, nc, cus), (nv, nc, cus)
        for ns in (1, 32):
            assert hpgv.score_plan_rows(nv, nc, ns, cus) == _score_rows(nv, nc, cus), (nv, nc, cus)


def test_ibs_plan_is_the_launch_arithmetic_it_was():
    band = 0
    for nv, nc, cus in _shapes():
        rows = hpgv.ibs_plan_rows(nv, nc, cus)
        if nv > 2 ** 31 - 64:
            # the rounded-up range of the inline arithmetic did not fit an int here: now two ranges or more
            assert rows > 0 and rows % 64 == 0, (nv, nc, cus, rows)
            band += 1
        else:
            assert rows == _ibs_rows(nv, nc, cus), (nv, nc, cus)
    assert band == 3
    # the shapes of tools/bench_ibs.py: one range where the tile pairs fill the device, ranges where they do not
    assert hpgv.ibs_plan_rows(100000, 10000, 256) == 100032 and hpgv.ibs_plan_rows(1000000, 200, 256) == _up(_up(1000000, 103), 64) * 64
