"""The principal components on the device (include/hpgv.h "PCA"): hpgv_grm_matrix_dev against the mirrored golden value with
array_equal, k_pca_apply against exact int64 products on both sides of every tile, k-step, block and panel edge with NaN in every
element of A it must not read, its values under the gamma_n bound, and hpgv_pca_dev against numpy under pca_golden's bounds."""
import ctypes as C

import numpy as np
import pytest

import grm_golden as gg
import ibs_golden as ig
import pca_golden as pg
from helpers import hpgv

pytestmark = pytest.mark.gpu

FILL = -12345.625                                                # what the tests leave where nothing may be written


@pytest.fixture(scope="module")
def eng():
    e = ig.engine()
    yield e
    e.close()


class Dev:
    """device buffers of a test, freed together"""

    def __init__(self, e):
        self.e, self.bufs = e, []

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        d = self.e.alloc(max(arr.nbytes, 16))
        self.e.h2d(d, arr)
        self.bufs.append(d)
        return d

    def close(self):
        for d in self.bufs:
            self.e.free(d)


def _padded(A, lda, fill=np.nan):
    """A [n, n] in rows of lda elements, `fill` past column n, and one more row of fill behind it"""
    n = len(A)
    out = np.full((n + 1, lda), fill, np.float64)
    out[:n, :n] = A
    return out


def _even(n):
    return (n + 1) & ~1


# ---- hpgv_grm_matrix_dev -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,rows", [(17, 64), (65, 65), (130, 300)])
def test_grm_matrix(eng, cols, rows):
    codes = ig.matrix(rows, cols).copy()
    codes[:, 3] = 0xFF                                           # an all-missing column: its diagonal and every pair with it are empty
    codes[0::2, 5] = 0xFF                                        # two columns missing on complementary rows: a pair that never meets
    codes[1::2, 9] = 0xFF
    s = gg.DEFAULT[0]
    acc = gg.golden(codes, *gg.DEFAULT)["acc"]
    exp, n_empty = pg.mirrored(acc, s)
    assert acc[5, 9, 1] == 0 and acc[5, 5, 1] > 0 and acc[9, 9, 1] > 0 and n_empty == cols + 1 and (exp[3] == 0).all() and exp[5, 9] == 0 and exp[9, 5] == 0
    buf = gg.fresh_acc(cols)
    buf[np.triu(np.ones((cols, cols), bool))] = acc[np.triu(np.ones((cols, cols), bool))]      # the lower half keeps gg.PATTERN
    for lda in (_even(cols), _even(cols) + 34):
        D = Dev(eng)
        d_acc, d_A, d_n = D.put(buf), D.put(np.full((cols, lda), FILL)), D.put(np.full(2, 0x77, np.uint64))
        eng.grm_matrix_dev(d_acc, cols, s, d_A, lda, d_n)
        eng.sync()
        got, n = eng.d2h(d_A, (cols, lda), np.float64), int(eng.d2h(d_n, (1,), np.uint64)[0])
        D.close()
        assert np.array_equal(got[:, :cols], exp), np.argwhere(got[:, :cols] != exp)[:4]
        assert np.array_equal(got[:, :cols], got[:, :cols].T) and (got[:, cols:] == FILL).all()
        assert n == n_empty
        keep = np.triu(np.ones((cols, cols), bool)) & (acc[..., 1] > 0)
        assert np.array_equal(got[:, :cols][keep], hpgv.grm_value(acc[keep], s))      # hpgv_grm_value's bits


def test_grm_matrix_refusals(eng):
    D = Dev(eng)
    d_acc, d_A, d_n = D.put(gg.fresh_acc(8)), D.put(np.zeros((8, 8))), D.put(np.zeros(2, np.uint64))
    bad = [dict(frac_bits=-1), dict(frac_bits=15), dict(lda=7), dict(lda=6), dict(lda=9), dict(d_acc=None), dict(d_A=None), dict(d_n=None),
           dict(d_acc=d_acc.value + 8), dict(d_A=d_A.value + 8), dict(d_n=d_n.value + 4), dict(n=-1)]
    for b in bad:
        a = dict(d_acc=d_acc, n=8, frac_bits=11, d_A=d_A, lda=8, d_n=d_n)
        a.update(b)
        with pytest.raises(hpgv.HpgvError, match="error %d" % hpgv.ERR_INVALID):
            eng.grm_matrix_dev(a["d_acc"], a["n"], a["frac_bits"], a["d_A"], a["lda"], a["d_n"])
    eng.grm_matrix_dev(d_acc, 0, 11, d_A, 8, d_n)                 # no columns: the counter is zeroed, nothing else
    eng.sync()
    D.close()


# ---- hpgv_pca_apply_dev --------------------------------------------------------------------------------------------------------
# 64: the panel and four blocks of 16 rows; 128 / 129: two whole panels, and a third of one row; 1030: 17 panels, the last ragged
SIZES = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 257, 1030]


def _apply(eng, A, Q, lda, tail=64):
    """Y [n, L] of hpgv_pca_apply_dev and the `tail` elements behind it, which were FILL"""
    n, L = Q.shape
    D = Dev(eng)
    d_A, d_Q, d_Y = D.put(_padded(A, lda)), D.put(Q), D.put(np.full(n * L + tail, FILL))
    eng.pca_apply_dev(d_A, n, lda, d_Q, L, d_Y)
    eng.sync()
    out = eng.d2h(d_Y, (n * L + tail,), np.float64)
    D.close()
    return out[: n * L].reshape(n, L), out[n * L:]


@pytest.mark.parametrize("L", [16, 32])
@pytest.mark.parametrize("n", SIZES)
def test_apply_exact(eng, n, L):
    """small integers: every product and every partial sum is exact in f64, so ANY summation order gives the int64 product.  A is
    symmetric but Q is not, and Q's columns differ: a swapped tile, row map or column map shows."""
    A = pg.integer_symmetric(n, -7, 7, 1000 + n)
    Q = np.random.default_rng(2000 + n + L).integers(-3, 4, (n, L))
    exp = (A @ Q).astype(np.float64)
    for lda in (_even(n), _even(n) + 34):
        Y, behind = _apply(eng, A.astype(np.float64), Q.astype(np.float64), lda)
        assert np.array_equal(Y, exp), "lda %d: differs at %s" % (lda, np.argwhere(Y != exp)[:4].tolist())
        assert (behind == FILL).all()


def test_apply_values_and_repeatability(eng):
    n = 257
    rng = np.random.default_rng(31)
    A = rng.standard_normal((n, n)) * 10.0 ** rng.uniform(-3, 3, (n, n))
    A = np.triu(A) + np.triu(A, 1).T
    for L in (16, 32):
        Q = rng.standard_normal((n, L))
        Y, _ = _apply(eng, A, Q, _even(n))
        bound = n * pg.EPS * (np.abs(A) @ np.abs(Q))                 # gamma_n: holds for every summation order
        assert (np.abs(Y - A @ Q) <= bound).all(), (np.abs(Y - A @ Q) / bound).max()
        again, _ = _apply(eng, A, Q, _even(n) + 34)
        assert np.array_equal(Y.view(np.uint64), again.view(np.uint64))


def test_apply_refusals(eng):
    D = Dev(eng)
    d_A, d_Q, d_Y = D.put(np.zeros((8, 8))), D.put(np.zeros((8, 16))), D.put(np.zeros((8, 16)))
    bad = [dict(L=8), dict(L=24), dict(L=64), dict(n=-1), dict(lda=7), dict(lda=6), dict(lda=9), dict(d_A=None), dict(d_Q=None), dict(d_Y=None),
           dict(d_A=d_A.value + 8), dict(d_Q=d_Q.value + 4), dict(d_Y=d_Y.value + 4)]
    for b in bad:
        a = dict(d_A=d_A, n=8, lda=8, d_Q=d_Q, L=16, d_Y=d_Y)
        a.update(b)
        with pytest.raises(hpgv.HpgvError, match="error %d" % hpgv.ERR_INVALID):
            eng.pca_apply_dev(a["d_A"], a["n"], a["lda"], a["d_Q"], a["L"], a["d_Y"])
    eng.pca_apply_dev(d_A, 0, 8, d_Q, 16, d_Y)
    eng.sync()
    D.close()


# ---- hpgv_pca_dev --------------------------------------------------------------------------------------------------------------
def _solve(eng, A, k, lda=None, **kw):
    n = len(A)
    lda = lda or _even(n) + 2
    D = Dev(eng)
    d_A = D.put(_padded(A, max(lda, n)))                         # (a refused pitch below n: the buffer is never read)
    try:
        return eng.pca_dev(d_A, n, lda, k, kw.pop("tol", pg.TOL), kw.pop("max_iter", pg.MAX_ITER), kw.pop("seed", pg.SEED))
    finally:
        D.close()


def _same(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ("eigval", "vec", "resid")) and (a["n_iter"], a["converged"]) == (b["n_iter"], b["converged"])


@pytest.mark.parametrize("name", pg.DEVICE_CASES)
def test_solver(eng, name):
    A, k = pg.case(name)
    out = _solve(eng, A, k)
    ref = pg.solved(name)
    print(name, "sweeps", out["n_iter"], "numpy", ref["n_iter"], "residuals", out["resid"])
    assert out["converged"] == 1 and abs(out["n_iter"] - ref["n_iter"]) <= 2
    pg.check_pairs(A, out, k, repeated=pg.REPEATED.get(name, ()))
    assert _same(out, _solve(eng, A, k)), "a second call differs"


@pytest.mark.parametrize("name", pg.HOST_CASES)
def test_solver_small_matrices_on_the_host(eng, name):
    A, k = pg.case(name)
    out = _solve(eng, A, k)
    assert out["n_iter"] == 0 and out["converged"] == 1
    pg.check_pairs(A, out, k, tol=pg.TOL)
    assert _same(out, _solve(eng, A, k))


def test_solver_stops_at_max_iter(eng):
    A, k = pg.case("population_130_10")
    out = _solve(eng, A, k, max_iter=1)
    assert out["converged"] == 0 and out["n_iter"] == 1
    res = pg.check_pairs(A, out, k, converged=False)
    assert res.max() > pg.TOL * np.abs(out["eigval"]).max()


def test_solver_refuses_a_matrix_of_low_rank(eng):
    with pytest.raises(hpgv.HpgvError, match="error %d.*rank" % hpgv.ERR_UNSUPPORTED):
        _solve(eng, pg.rank3(), 10)


def test_solver_refusals(eng):
    A = pg.case("negative_65_3")[0]
    for kw in (dict(k=0), dict(k=-1), dict(k=25), dict(k=66), dict(tol=0.0), dict(tol=-1e-8), dict(tol=float("nan")), dict(tol=float("inf")),
               dict(max_iter=0), dict(max_iter=-5), dict(lda=65), dict(lda=64)):
        a = dict(k=3)
        a.update(kw)
        with pytest.raises(hpgv.HpgvError, match="error %d" % hpgv.ERR_INVALID):
            _solve(eng, A, **a)
    D = Dev(eng)
    d_A = D.put(_padded(A, 66))
    val, vec, res, it, conv = np.zeros(3), np.zeros((65, 3)), np.zeros(3), C.c_int(0), C.c_int(0)
    P = lambda a: a.ctypes.data
    full = [d_A, 65, 66, 3, 1e-8, 10, 1, P(val), P(vec), P(res), C.byref(it), C.byref(conv)]
    for at in (0, 7, 8, 9, 10, 11):                                # each pointer NULL in turn
        args = list(full)
        args[at] = None
        assert eng.L.hpgv_pca_dev(eng.h, *args) == hpgv.ERR_INVALID, at
    assert eng.L.hpgv_pca_dev(eng.h, d_A.value + 8, 65, 66, 3, 1e-8, 10, 1, P(val), P(vec), P(res), C.byref(it), C.byref(conv)) == hpgv.ERR_INVALID
    D.close()
