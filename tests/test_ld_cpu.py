"""The LD band without a device: the new symbols are exported, hpgv_ld_r2 is the header's expression bit for bit, and the golden of
the GPU tests agrees with numpy's corrcoef over the jointly called samples."""
import os
import re

import numpy as np

import ld_golden as lg
from helpers import hpgv
from model_golden import bits, classes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_window_limit():
    L = hpgv.load()
    for name in ("hpgv_ld_window_dev", "hpgv_ld", "hpgv_ld_text", "hpgv_ld_r2"):
        assert name in hpgv.SYMBOLS and hasattr(L, name)
    text = open(os.path.join(ROOT, "include", "hpgv.h")).read()
    assert int(re.search(r"#define HPGV_LD_MAX_WINDOW (\d+)", text).group(1)) == 1024 == max(lg.WINDOWS)


def test_ld_r2_is_the_expression_bit_for_bit():
    rng = np.random.default_rng(41)
    # moments of random dosage rows of up to 100 000 samples: every count a real one, the differences up to 2^36
    rows = []
    for _ in range(300):
        ns = int(rng.integers(1, 100001))
        ga, gb = rng.integers(0, 3, ns), rng.integers(0, 3, ns)
        va, vb = rng.random(ns) < rng.uniform(0.5, 1.0), rng.random(ns) < rng.uniform(0.5, 1.0)
        ga, gb, j = ga * va, gb * vb, (va & vb).astype(np.int64)
        rows.append([j.sum(), (ga * j).sum(), (gb * j).sum(), (ga * ga * j).sum(), (gb * gb * j).sum(), (ga * gb).sum()])
    # and count vectors that are no moments of anything: the function evaluates the expression, whatever it is given
    c6 = np.concatenate([np.array(rows, np.int64), rng.integers(0, 1 << 22, size=(300, 6))]).astype(np.int32)
    got, exp = hpgv.ld_r2(c6), lg.r2_of(c6)
    assert np.isfinite(exp).sum() >= 590
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    assert np.array_equal(bits(got)[ok], bits(exp)[ok])
    # the NaN cases: n = 0; n = 1; a monomorphic first row (all 0, all 1, all 2); a monomorphic second row; both
    nan = np.array([[0, 0, 0, 0, 0, 0], [1, 1, 2, 1, 4, 2], [50, 0, 40, 0, 60, 0], [50, 50, 40, 50, 60, 40], [50, 100, 40, 200, 60, 80],
                    [50, 40, 0, 60, 0, 0], [50, 100, 100, 200, 200, 200]], np.int32)
    assert np.isnan(hpgv.ld_r2(nan)).all() and np.isnan(lg.r2_of(nan)).all()
    # a copy and a mirror image of a row: exactly 1, the mirror with a negative covariance
    one = np.array([[60, 70, 70, 110, 110, 110], [60, 70, 50, 110, 70, 30]], np.int32)
    assert np.array_equal(hpgv.ld_r2(one), [1.0, 1.0])
    assert 60 * 30 - 70 * 50 < 0


def test_golden_agrees_with_corrcoef():
    defined = total = 0
    for width, nv, window in (((37, 45), 150, 10), ((301, 412), 65, 64), ((64, 64), 300, 3)):
        codes = lg.matrix(width, nv)
        r2, c6, inband = lg.golden(width, nv, window)
        valid, dosage = classes(codes)
        for b in range(nv):
            for d in range(1, min(window, b) + 1):
                a = b - d
                j = valid[a] & valid[b]
                x, y = dosage[a, j].astype(np.float64), dosage[b, j].astype(np.float64)
                assert c6[b, d - 1, 0] == j.sum() and c6[b, d - 1, 5] == (dosage[a] * dosage[b]).sum()
                total += 1
                if j.sum() < 2 or x.std() == 0 or y.std() == 0:
                    assert np.isnan(r2[b, d - 1])
                    continue
                defined += 1
                rho = np.corrcoef(x, y)[0, 1]
                # 1e-12 relative, plus what corrcoef itself can be off by: it subtracts floating-point means and sums n products in
                # float64, so its rho carries an absolute error of up to dr = n eps (the bound of an n-term dot product relative to
                # |x| |y|), and rho^2 one of 2 |rho| dr + dr^2.  The golden's own integers are exact; without this term no correct
                # golden passes where the covariance is 0 or a few units (rho around 1e-5: corrcoef keeps 12 digits of it at best)
                dr = j.sum() * np.finfo(np.float64).eps
                assert abs(r2[b, d - 1] - rho * rho) <= 1e-12 * r2[b, d - 1] + 2 * abs(rho) * dr + dr * dr, (width, b, d, r2[b, d - 1], rho * rho)
        # what lies before the first row is outside the band
        assert all(np.isnan(r2[b, b:]).all() and not inband[b, b:].any() for b in range(min(nv, window)))
    assert defined >= 0.95 * total and total > 4000, (defined, total)
