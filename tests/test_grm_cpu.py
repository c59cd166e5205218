"""The genetic relationship matrix without a device (include/hpgv.h "GRM"): the new symbols are exported, hpgv_grm_table is the
header's expressions bit for bit, the limbs recombine, hpgv_grm_frac_bits and hpgv_grm_value are the header's, no row range of the
launch plan can overflow an i32 sum, and the quantised matrix lies within the derived bound of the unquantised one."""
import numpy as np
import pytest

import grm_golden as gg
import ibs_golden as ig
from helpers import hpgv, random_codes
from model_golden import bits, classes


@pytest.fixture(scope="module", autouse=True)
def built():
    hpgv.build()


def test_symbols_are_exported():
    L = hpgv.load()
    for name in ("hpgv_grm_table_dev", "hpgv_grm_pairs_dev", "hpgv_grm", "hpgv_grm_text", "hpgv_grm_table", "hpgv_grm_frac_bits", "hpgv_grm_value",
                 "hpgv_grm_plan_rows"):
        assert name in hpgv.SYMBOLS and hasattr(L, name)
    assert hpgv.GRM_ACC.itemsize == 16 and hpgv.GRM_ACC.fields["n"][1] == 8 and hpgv.GRM_TAB.itemsize == 8 and hpgv.GRM_TAB.fields["lo"][1] == 4
    for name in ("grm_table", "grm_frac_bits", "grm_value", "run_grm"):
        assert callable(getattr(hpgv, name))
    for name in ("grm_table_dev", "grm_pairs_dev", "grm_text"):
        assert callable(getattr(hpgv.Engine, name))


def _sweep():
    """class counts [rows, 3]: every small cohort, Y = 0, Y = T, a single column, MAF on both sides of the thresholds, n up to 2^20"""
    rows = [(a, b, c) for a in range(6) for b in range(6) for c in range(6)]
    rows += [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]                                   # a single column, none
    rows += [(50, 0, 0), (0, 0, 50), (0, 50, 0)]                                           # Y = 0, Y = T, every call heterozygous
    for n in (100, 1000, 4097, 1 << 20):
        for y in (1, 2, n // 100, n // 100 + 1, 2 * n // 100 - 1, 2 * n // 100, 2 * n // 100 + 1, n // 10, n // 2, n, 2 * n - 2 * n // 100, 2 * n - 1):
            for n2 in (0, y // 4, y // 2):                                                 # Y = n1 + 2 n2 alternate alleles among 2 n
                n1 = y - 2 * n2
                if n1 >= 0 and n - n1 - n2 >= 0:
                    rows.append((n - n1 - n2, n1, n2))
    rng = np.random.default_rng(8)
    rows += rng.integers(0, 3000, (300, 3)).tolist()
    rows += [(-1, 5, 5), (5, -1, 5), (5, 5, -1)]                                           # a negative count is no row
    return np.array(rows, np.int64)


@pytest.mark.parametrize("frac_bits,min_maf", [(11, 0.01), (14, 0.5), (12, 0.05), (0, 0.0), (14, 0.01), (9, 0.001)])
def test_table_is_the_expression_bit_for_bit(frac_bits, min_maf):
    c = _sweep()
    used, tab = hpgv.grm_table(c, frac_bits, min_maf)
    exp_used, q = gg.table(c, frac_bits, min_maf)
    exp = gg.tab_records(exp_used, q)
    assert np.array_equal(used, exp_used)
    assert np.array_equal(tab["hi"], exp["hi"]) and np.array_equal(tab["lo"], exp["lo"])
    # 256 hi + lo == q, hi inside +-127, entry 3 and every unused row zero
    hi, lo = tab["hi"].astype(np.int64), tab["lo"].astype(np.int64)
    assert np.array_equal(256 * hi[:, :3] + lo[:, :3], q) and np.abs(hi).max() <= 127
    assert not hi[:, 3].any() and not lo[:, 3].any() and not hi[~used].any() and not lo[~used].any()
    assert used.any() and (~used).any()
    X, Y = 2 * c[:, 0] + c[:, 1], c[:, 1] + 2 * c[:, 2]
    assert not used[(Y <= 0) | (Y >= X + Y) | (c < 0).any(axis=1)].any()
    if min_maf > 0:
        ok = (c >= 0).all(axis=1) & (X + Y > 0)
        maf = np.minimum(X, Y)[ok] / (X + Y)[ok].astype(np.float64)
        assert (maf[used[ok]] >= min_maf).all() and (maf >= min_maf).any() and (maf < min_maf).any()
    if (frac_bits, min_maf) == (14, 0.01):
        # a frac_bits too large for the MAF: the rows whose q would leave 16 bits (|q| > 32512) are unused, the others stay
        _, q11 = gg.table(c, 11, min_maf)
        lost = (np.abs(q11).max(axis=1) * 8 > gg.MAX_Q + 8) & gg.table(c, 11, min_maf)[0]
        assert lost.any() and not used[lost].any() and used.any()
    if min_maf > 0 and frac_bits == hpgv.grm_frac_bits(min_maf):
        # at the recommended frac_bits no row is lost to the |q| rule
        assert np.array_equal(used, gg.table(c, 0, min_maf)[0])


def test_frac_bits():
    assert [hpgv.grm_frac_bits(m) for m in (0.5, 0.1, 0.05, 0.01, 0.001)] == [14, 12, 12, 11, 9]
    for m in (0.0, -0.1, 0.5000001, 1.0, float("nan"), float("inf")):
        assert hpgv.grm_frac_bits(m) == -1
    for m in (0.5, 0.3, 0.1, 0.02, 0.001, 1e-5):
        s = hpgv.grm_frac_bits(m)
        z = np.sqrt(2.0 * (1.0 - m) / m)
        assert z * 2.0 ** s <= gg.MAX_Q and (s == 14 or z * 2.0 ** (s + 1) > gg.MAX_Q)


def test_value_is_the_expression_bit_for_bit():
    rng = np.random.default_rng(3)
    acc = np.stack([rng.integers(-(1 << 50), 1 << 50, 400), rng.integers(1, 1 << 30, 400)], axis=-1)
    acc = np.concatenate([acc, [[0, 0], [5, 0], [-5, 0], [0, 7], [(1 << 62), 1], [-(1 << 62), 3]]]).astype(np.int64)
    for s in (0, 9, 11, 14):
        got, exp = hpgv.grm_value(acc, s), gg.value(acc, s)
        ig.same_bits(got, exp, "value at %d" % s)
        assert np.isnan(got[400]) and np.isposinf(got[401]) and np.isneginf(got[402]) and got[403] == 0.0
    st = np.zeros(len(acc), hpgv.GRM_ACC)
    st["sq"], st["n"] = acc.T
    assert np.array_equal(bits(hpgv.grm_value(st[:400], 11)), bits(gg.value(acc[:400], 11)))


def test_no_row_range_overflows_an_i32_sum():
    """per row |hi_i lo_j + lo_i hi_j| <= 2 * 127 * 128 = 32 512, so a range of at most 32 768 rows stays below 2^31"""
    assert 32768 * 2 * 127 * 128 < 2 ** 31
    shapes = [(10 ** 6, 3000, 256), (70000, 20, 256), (2 ** 31 - 1, 1, 256), (2 ** 31 - 1, 100000, 256), (2 ** 31 - 1, 3000, 1), (0, 0, 0), (1, 1, 1),
              (32769, 3000, 256), (65536, 5000, 304), (66053, 2048, 64)]
    rng = np.random.default_rng(4)
    shapes += [(int(10 ** rng.uniform(0, 9.3)), int(10 ** rng.uniform(0, 5)), int(rng.integers(1, 400))) for _ in range(300)]
    for nv, nc, cus in shapes:
        rows = hpgv.grm_plan_rows(nv, nc, cus)
        assert 64 <= rows <= 32768 and rows % 64 == 0, (nv, nc, cus, rows)
    # many columns, where IBS's plan makes ONE range of all rows: as few ranges as the cap allows, and EQUAL ones -- the grid deals
    # contiguous runs of (range, pair) items to the XCDs, so a short last range would idle the XCDs that draw it
    for nv, nc in ((10 ** 6, 3000), (100000, 10000), (32832, 10000), (65537, 4096)):
        rows = hpgv.grm_plan_rows(nv, nc, 256)
        ranges = -(-nv // rows)
        assert ranges == -(-nv // 32768) and nv - (ranges - 1) * rows > rows - 64 * ranges, (nv, nc, rows)
    assert hpgv.grm_plan_rows(32768, 10000, 256) == 32768
    assert hpgv.grm_plan_rows(70000, 20, 256) < 16384            # few columns: the ranges fill the device


def test_quantised_matrix_is_within_the_derived_bound():
    """|q_c 2^-s - z_c| <= delta = 2^-(s+1), so |q_i q_j 2^-2s - z_i z_j| <= delta (|z_i| + |z_j|) + delta^2 per row, and a pair's
    value lies within the mean of that over its n rows of the unquantised one.  Derived, not measured; the unquantised sums are
    taken in long double so that their own rounding (2^-64 relative) stays far below the bound."""
    rng = np.random.default_rng(21)
    codes = random_codes(rng, 300, 130, quirks=False, strict=False, p_missing=0.03)
    for frac_bits, min_maf in ((11, 0.01), (14, 0.5 - 0.2), (9, 0.001)):
        G = gg.golden(codes, frac_bits, min_maf)
        assert G["used"].sum() > 100
        valid, g = classes(codes)
        V = valid & G["used"][:, None]
        z = gg.z_table(G["class4"], min_maf)
        Z = np.where(V, np.take_along_axis(z, g, axis=1), np.longdouble(0))
        n = (V.astype(np.int64).T @ V.astype(np.int64))
        exact = (Z.T @ Z) / n
        delta = np.longdouble(2.0) ** -(frac_bits + 1)
        absZ, Vl = np.abs(Z), V.astype(np.longdouble)
        bound = (delta * (absZ.T @ Vl + Vl.T @ absZ) + delta * delta * n) / n
        iu = np.triu_indices(codes.shape[1])
        dev = np.abs(gg.value(G["acc"], frac_bits).astype(np.longdouble) - exact)[iu]
        print("frac_bits %d: largest deviation %.3g, %.3g of its bound" % (frac_bits, float(dev.max()), float((dev / bound[iu]).max())))
        assert (n[iu] > 0).all() and (dev <= bound[iu]).all()
        # and the golden's limbs carry its q: the identity the kernel's epilogue uses
        hi, lo = gg.limbs(np.take_along_axis(G["q"], g, axis=1) * V)
        sq = 65536 * (hi.T @ hi) + 256 * (hi.T @ lo + lo.T @ hi) + lo.T @ lo
        assert np.array_equal(sq[iu], G["acc"][..., 0][iu]) and np.abs(hi).max() <= 127
