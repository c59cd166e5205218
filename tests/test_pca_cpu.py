"""The host pieces of the principal components (include/hpgv.h "PCA"), which need no device: the exported symbols, the block
width, the cyclic Jacobi eigen-solver and the Cholesky factor's inverse against LAPACK under pca_golden.small_bound, and the
sweep counts of the numpy iteration on every matrix the GPU tests solve."""
import numpy as np
import pytest

import pca_golden as pg
from helpers import hpgv

NEW = ["hpgv_grm_matrix_dev", "hpgv_pca_apply_dev", "hpgv_pca_dev", "hpgv_pca_block", "hpgv_pca_jacobi", "hpgv_pca_chol_inv"]


@pytest.fixture(scope="module", autouse=True)
def built():
    hpgv.build()


def test_the_symbols_are_exported_and_listed():
    L = hpgv.load()
    for name in NEW:
        assert name in hpgv.SYMBOLS and hasattr(L, name), name


def test_block_width():
    assert [hpgv.pca_block(k) for k in (-1, 0, 1, 8, 9, 24, 25, 1000)] == [-1, -1, 16, 16, 32, 32, -1, -1]
    assert all(hpgv.pca_block(k) == pg.block(k) for k in range(1, 25))


def _symmetric_inputs():
    rng = np.random.default_rng(77)
    out = {}
    for L in (1, 2, 3, 16, 32):
        H = rng.standard_normal((L, L))
        out["random_%d" % L] = H + H.T
        U, _ = np.linalg.qr(rng.standard_normal((L, L)))
        lam = np.arange(1, L + 1, dtype=np.float64)
        lam[: (L + 1) // 2] = 3.0                                   # a repeated eigenvalue
        out["repeated_%d" % L] = (U * lam) @ U.T
        out["diagonal_%d" % L] = np.diag(rng.standard_normal(L) * 10.0 ** rng.integers(-3, 4, L))
        out["zero_%d" % L] = np.zeros((L, L))
        out["negative_definite_%d" % L] = -((U * (lam + 1.0)) @ U.T)
    return out


SYMMETRIC = _symmetric_inputs()


def _figures(H, theta, W):
    L = len(H)
    return np.linalg.norm(H @ W - W * theta), np.linalg.norm(W.T @ W - np.eye(L))


@pytest.mark.parametrize("name", sorted(SYMMETRIC))
def test_jacobi_against_lapack(name):
    """Residual ||H W - W Theta||_F and orthogonality defect ||W^T W - I||_F within 8 x max(LAPACK's own, L eps ||H||_F); the
    eigenvalues within the same bound of eigh's; the pairs by decreasing |theta|.  Largest ratios observed to max(LAPACK's own,
    L eps ||H||_F): residual 0.4; orthogonality, against max(LAPACK's own, L eps): 4.0 (L = 32) -- of the margin of 8."""
    H = (SYMMETRIC[name] + SYMMETRIC[name].T) / 2
    L = len(H)
    theta, W = hpgv.pca_jacobi(H)
    w, V = np.linalg.eigh(H)
    r, o = _figures(H, theta, W)
    rl, ol = _figures(H, w, V)
    print("%s: residual %.3g (LAPACK %.3g), orthogonality %.3g (LAPACK %.3g), L eps |H| %.3g" % (name, r, rl, o, ol, L * pg.EPS * np.linalg.norm(H)))
    assert r <= pg.small_bound(L, H, rl) and o <= 8 * max(ol, L * pg.EPS * min(1.0, np.linalg.norm(H)))      # (the defect has no scale: never looser than L eps)
    assert np.abs(np.sort(theta) - w).max() <= pg.small_bound(L, H, rl)
    assert (np.diff(np.abs(theta)) <= 0).all()


def test_jacobi_symmetrises_and_refuses():
    H = np.array([[2.0, 1.0], [3.0, -1.0]])
    theta, W = hpgv.pca_jacobi(H)
    assert np.allclose(np.sort(theta), np.linalg.eigvalsh((H + H.T) / 2), rtol=0, atol=1e-14)
    L = hpgv.load()
    buf = np.zeros(33 * 33)
    assert L.hpgv_pca_jacobi(0, buf.ctypes.data, buf.ctypes.data) == hpgv.ERR_INVALID
    assert L.hpgv_pca_jacobi(33, buf.ctypes.data, buf.ctypes.data) == hpgv.ERR_INVALID
    assert L.hpgv_pca_jacobi(4, None, buf.ctypes.data) == hpgv.ERR_INVALID


@pytest.mark.parametrize("L", [1, 2, 3, 16, 32])
def test_chol_inv(L):
    """||M^T G M - I||_F within 8 x max(LAPACK's route on the same input, L eps ||I||_F); M is upper triangular"""
    rng = np.random.default_rng(100 + L)
    B = rng.standard_normal((3 * L, L))
    G = B.T @ B
    failed, M = hpgv.pca_chol_inv(G)
    assert not failed and np.array_equal(M, np.triu(M))
    Ml = np.linalg.inv(np.linalg.cholesky(G).T)
    eye = np.eye(L)
    got, lapack = np.linalg.norm(M.T @ G @ M - eye), np.linalg.norm(Ml.T @ G @ Ml - eye)
    print("L %d: %.3g (LAPACK %.3g)" % (L, got, lapack))
    assert got <= pg.small_bound(L, eye, lapack)


def test_chol_inv_reports_a_failed_pivot():
    rng = np.random.default_rng(5)
    B = rng.standard_normal((16, 3))
    singular = B @ B.T                                              # rank 3 of 16
    indefinite = np.diag([4.0, 1.0, -2.0, 3.0])
    for G in (singular, indefinite, np.zeros((5, 5)), np.ones((3, 3)), np.full((2, 2), np.nan)):
        assert hpgv.pca_chol_inv(G)[0]
    assert not hpgv.pca_chol_inv(np.eye(32))[0]
    L = hpgv.load()
    buf = np.zeros(33 * 33)
    assert L.hpgv_pca_chol_inv(33, buf.ctypes.data, buf.ctypes.data) == -1 and L.hpgv_pca_chol_inv(3, None, buf.ctypes.data) == -1


def test_the_start_block_is_spread_and_fixed():
    Q = pg.start_block(257, 32, pg.SEED)
    assert Q.min() >= -0.5 and Q.max() < 0.5 and abs(Q.mean()) < 0.01 and len(np.unique(Q)) == Q.size
    assert np.array_equal(Q[:130, :16], pg.start_block(130, 32, pg.SEED)[:, :16])      # a function of (seed, row, column)
    assert np.linalg.cond(Q) < 3


@pytest.mark.parametrize("name", pg.DEVICE_CASES)
def test_inputs_stay_inside_the_iteration_cap(name):
    """every matrix the GPU tests solve converges in numpy at their tol within HALF their max_iter: 8-9 sweeps for the planted
    spectra, 42-46 for the three planted groups at 130 samples"""
    out = pg.solved(name)
    print(name, out["n_iter"])
    assert out["converged"] == 1 and 1 <= out["n_iter"] <= pg.MAX_ITER // 2
    A, k = pg.case(name)
    pg.check_pairs(A, out, k, repeated=pg.REPEATED.get(name, ()))


def test_the_runner_input_stays_inside_its_cap():
    """the runner tests' cohort at the runner's constants (tol 1e-8, 1 000 sweeps at most, seed 1): 61 sweeps in numpy"""
    R = pg.RUNNER
    A = pg.runner_golden(hpgv.grm_frac_bits(R["min_maf"]))[1]
    out = pg.iterate(A, R["k"], R["tol"], R["max_iter"], R["seed"])
    print("runner cohort", out["n_iter"])
    assert out["converged"] == 1 and out["n_iter"] <= R["max_iter"] // 2
    pg.check_pairs(A, out, R["k"], tol=R["tol"])


def test_a_rank_deficient_block_fails_in_numpy_too():
    assert pg.iterate(pg.rank3(), 10) is None
