"""Goldens of the principal components (include/hpgv.h "PCA"): the header's iteration in numpy -- the same start block, CholQR done
twice with numpy.linalg.cholesky, numpy.linalg.eigh for the Rayleigh-Ritz step, the explicit residual block --, the matrices the
tests solve (planted spectra, the GRM of planted populations, exact small-integer matrices), the cases the GPU tests and the CPU
test of their sweep counts share, and the bounds."""
import functools

import numpy as np

import grm_golden as gg

EPS = float(np.finfo(np.float64).eps)
TOL, MAX_ITER, SEED = 1e-8, 200, 7
M64 = (1 << 64) - 1


def block(k):
    return 16 if 1 <= k <= 8 else 32 if k <= 24 else -1


def start_block(n, L, seed):
    """the header's start block: splitmix64's finaliser of seed + golden (32 row + col + 1), top 53 bits as a fraction, minus 0.5"""
    with np.errstate(over="ignore"):
        ctr = (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(32) + np.arange(L, dtype=np.uint64)[None, :] + np.uint64(1))
        x = np.uint64(seed & M64) + np.uint64(0x9E3779B97F4A7C15) * ctr
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5


def _orth(Y):
    """CholQR done twice; None when a factorisation fails"""
    for _ in range(2):
        try:
            R = np.linalg.cholesky(Y.T @ Y).T
        except np.linalg.LinAlgError:
            return None
        Y = np.linalg.solve(R.T, Y.T).T
    return Y


def normalise(x):
    x = x / np.linalg.norm(x)
    return -x if x[np.argmax(np.abs(x))] < 0 else x


def result_order(theta, k):
    """of the pairs by decreasing |theta| the first k, by decreasing theta"""
    first = np.argsort(-np.abs(theta), kind="stable")[:k]
    return first[np.argsort(-theta[first], kind="stable")]


def iterate(A, k, tol=TOL, max_iter=MAX_ITER, seed=SEED):
    """the header's solver in numpy: dict of eigval, vec, resid, n_iter, converged (None when the block loses rank)"""
    A = np.asarray(A, np.float64)
    n, L = len(A), block(k)
    if n <= L:
        w, V = np.linalg.eigh(A)
        o = result_order(w, k)
        X = np.stack([normalise(V[:, p]) for p in o], axis=1)
        res = np.linalg.norm(A @ X - X * w[o], axis=0)
        return dict(eigval=w[o], vec=X, resid=res, n_iter=0, converged=1)
    Q = _orth(start_block(n, L, seed))
    for it in range(1, max_iter + 1):
        Y = A @ Q
        H = Q.T @ Y
        theta, W = np.linalg.eigh((H + H.T) / 2)
        by = np.argsort(-np.abs(theta), kind="stable")
        theta, W = theta[by], W[:, by]
        res = np.linalg.norm(Y @ W - (Q @ W) * theta, axis=0)
        done = res[:k].max() <= tol * np.abs(theta[0])
        if done or it == max_iter:
            o = result_order(theta, k)
            X = np.stack([normalise((Q @ W)[:, p]) for p in o], axis=1)
            return dict(eigval=theta[o], vec=X, resid=res[o], n_iter=it, converged=int(done))
        Q = _orth(Y)
        if Q is None:
            return None


# ---- matrices ------------------------------------------------------------------------------------------------------------------
def planted_spectrum(n, top, bulk, seed):
    """(A, lam): U diag(lam) U^T with a random orthogonal U; lam = the planted `top` values and n - len(top) values uniform in
    [-bulk, bulk] (so the matrix has full rank and the block keeps its columns)"""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.concatenate([np.asarray(top, np.float64), rng.uniform(-bulk, bulk, n - len(top))])
    A = (U * lam) @ U.T
    return (A + A.T) / 2, lam


def population_codes(n_samples, n_variants, n_groups, seed, p_missing=0.01):
    """(codes [variants, samples] HPGV8 bytes, group [samples]): samples dealt to groups in turn, per group and variant the allele
    frequency clip(p + N(0, 0.25), 0.05, 0.95) of a base p in [0.1, 0.9], genotypes binomial, a few missing calls"""
    rng = np.random.default_rng(seed)
    group = np.arange(n_samples) % n_groups
    p = rng.uniform(0.1, 0.9, n_variants)
    pg = np.clip(p[:, None] + rng.normal(0.0, 0.25, (n_variants, n_groups)), 0.05, 0.95)
    f = pg[:, group]
    a, b = rng.random((n_variants, n_samples)) < f, rng.random((n_variants, n_samples)) < f
    codes = (a.astype(np.uint8) << 4) | b.astype(np.uint8)
    codes[rng.random(codes.shape) < p_missing] = 0xFF
    return codes, group


def mirrored(acc, frac_bits):
    """the full f64 matrix of upper-half sums [n, n, 2]: hpgv_grm_matrix_dev's result, 0.0 where n = 0; and the count of those"""
    up = np.triu(np.ones(acc.shape[:2], bool))
    val = gg.value(acc, frac_bits)
    empty = up & (acc[..., 1] == 0)
    val = np.where(up & ~empty, val, 0.0)
    return val + np.triu(val, 1).T, int(empty.sum())


@functools.lru_cache(maxsize=None)
def population_grm(n_samples=130, n_variants=400, n_groups=3, seed=11):
    codes, _ = population_codes(n_samples, n_variants, n_groups, seed)
    A, empty = mirrored(gg.golden(codes, *gg.DEFAULT)["acc"], gg.DEFAULT[0])
    assert empty == 0
    A.setflags(write=False)
    return A


RUNNER = dict(samples=60, variants=600, groups=3, k=4, min_maf=0.05, tol=1e-8, max_iter=1000, seed=1)      # the last three: include/hpgv_host.h


@functools.lru_cache(maxsize=None)
def runner_cohort():
    """the VCF of tests/test_pca_runner_gpu.py: (codes [variants, samples], group [samples], on_x [variants], mono, rare) -- three
    planted groups with missing calls, "1/2", monomorphic rows, rows below min_maf and chromosome-X rows"""
    NS, NV = RUNNER["samples"], RUNNER["variants"]
    rng = np.random.default_rng(47)
    codes, group = population_codes(NS, NV, RUNNER["groups"], 48, p_missing=0.03)
    codes[rng.random((NV, NS)) < 0.01] = 0x12                    # a few "1/2"
    mono = [7, 63, 64, 301]                                      # monomorphic rows, of either allele, one with missing genotypes
    codes[mono[:2]] = 0x00
    codes[mono[2:]] = 0x11
    codes[301, ::5] = 0xFF
    rare = [9, 100, 433]                                         # below min_maf: one, two and four alternate alleles among 120
    codes[rare] = 0x00
    codes[9, 4], codes[100, [4, 30]], codes[433, [1, 2]] = 0x01, 0x01, 0x11
    on_x = np.zeros(NV, bool)
    on_x[[0, 5, 299, 300, 599]] = True
    on_x[rng.random(NV) < 0.05] = True
    on_x[mono + rare] = False
    codes.setflags(write=False)
    return codes, group, on_x, mono, rare


def runner_golden(frac_bits):
    """(the golden of the runner's cohort, its mirrored f64 matrix)"""
    codes, _, on_x, _, _ = runner_cohort()
    G = gg.golden(codes, frac_bits, RUNNER["min_maf"], on_x.astype(np.uint8))
    A, empty = mirrored(G["acc"], frac_bits)
    assert empty == 0
    return G, A


def integer_symmetric(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    A = rng.integers(lo, hi + 1, (n, n))
    A = np.triu(A) + np.triu(A, 1).T
    return A.astype(np.int64)


# ---- the solver's cases: name -> (matrix, k); `repeated`: the indices (in the result) of a repeated eigenvalue ------------------
@functools.lru_cache(maxsize=None)
def case(name):
    if name == "spectrum_130_3":
        A = planted_spectrum(130, [50.0, 30.0, 20.0], 2.0, 1)[0]
        return A, 3
    if name == "spectrum_257_10":
        return planted_spectrum(257, np.linspace(100.0, 55.0, 10), 3.0, 2)[0], 10
    if name == "negative_65_3":
        return planted_spectrum(65, [-60.0, 40.0, 25.0], 2.0, 3)[0], 3
    if name == "repeated_33_8":
        return planted_spectrum(33, [40.0, 40.0, 30.0, 25.0, 20.0, 15.0, 12.0, 10.0], 1.0, 4)[0], 8
    if name == "population_130_3":
        return population_grm(), 3
    if name == "population_130_10":
        return population_grm(), 10
    if name.startswith("host_"):
        n = int(name[5:])
        k = 10 if n == 32 else min(3, n)
        return planted_spectrum(n, [9.0, -7.0, 5.0][:min(3, n)], 1.0, 50 + n)[0], k
    raise KeyError(name)


DEVICE_CASES = ["spectrum_130_3", "spectrum_257_10", "negative_65_3", "repeated_33_8", "population_130_3", "population_130_10"]
HOST_CASES = ["host_1", "host_5", "host_16", "host_32"]
REPEATED = {"repeated_33_8": (0, 1)}


@functools.lru_cache(maxsize=None)
def solved(name):
    A, k = case(name)
    return iterate(A, k)


def rank3(n=100, seed=9):
    rng = np.random.default_rng(seed)
    B = rng.integers(-3, 4, (n, 3)).astype(np.float64)
    return B @ B.T


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def residual_bound(A, theta, tol=TOL, extra=0.0):
    """||A x - theta x|| of a converged pair: the solver's own test, plus the rounding of the two products that measure it (the
    solver's and the test's), 4 n eps ||A||_F"""
    return tol * np.abs(theta).max() + 4 * len(A) * EPS * np.linalg.norm(A) + extra


def small_bound(L, H, lapack):
    """8 x max(LAPACK's own figure on the same input, L eps ||H||_F): both methods are backward stable with different constants"""
    return 8 * max(lapack, L * EPS * np.linalg.norm(H))


def check_pairs(A, out, k, tol=TOL, converged=True, repeated=(), extra=0.0, extra_orth=0.0, L=None):
    """the checks every solved case shares: recomputed residuals, the residual theorem, the k of largest magnitude in decreasing
    order, Davis-Kahan against numpy's vectors where the eigenvalue is simple, orthonormality, the sign rule"""
    A = np.asarray(A, np.float64)
    n = len(A)
    val, X = out["eigval"], out["vec"]
    assert val.shape == (k,) and X.shape == (n, k)
    res = np.linalg.norm(A @ X - X * val, axis=0)
    noise = 4 * n * EPS * np.linalg.norm(A) + extra
    if "resid" in out:                                   # (extra, extra_orth: what a caller's rounding of the pairs adds)
        assert (np.abs(res - out["resid"]) <= noise + 1e-10 * res).all(), "the returned residuals are not the true ones: %s against %s" % (out["resid"], res)
    lam, V = np.linalg.eigh(A)
    L = L or block(k)
    assert np.abs(X.T @ X - np.eye(k)).max() <= 64 * L * EPS + extra_orth, np.abs(X.T @ X - np.eye(k)).max()
    for c in range(k):
        assert X[np.argmax(np.abs(X[:, c])), c] > 0, "sign rule, vector %d" % c
    assert (np.diff(val) <= 0).all()
    if not converged:
        return res
    assert (res <= residual_bound(A, val, tol, extra)).all(), (res, residual_bound(A, val, tol, extra))
    want = lam[result_order(lam, k)]
    for c in range(k):
        assert np.abs(lam - val[c]).min() <= res[c] + noise, "residual theorem, pair %d" % c
        assert abs(want[c] - val[c]) <= res[c] + noise, "pair %d: %r is not the eigenvalue %r" % (c, val[c], want[c])
    for c in range(k):
        if c in repeated or n == 1:
            continue
        at = int(np.argmin(np.abs(lam - val[c])))
        gap = np.abs(np.delete(lam, at) - val[c]).min()
        sine = np.linalg.norm(X[:, c] - V[:, at] * (V[:, at] @ X[:, c]))
        # (numpy's own vector is within about n eps ||A|| / gap of the true one: the noise term)
        assert sine <= (res[c] + noise) / gap, "Davis-Kahan, pair %d: sine %g, residual %g, gap %g" % (c, sine, res[c], gap)
    if repeated:
        at = [int(np.argmin(np.abs(lam - val[c]))) for c in repeated]
        lo, hi = min(at), max(at)
        idx = [i for i in range(n) if abs(lam[i] - val[repeated[0]]) <= res[list(repeated)].max() + noise + 1e-9 * abs(val[repeated[0]])]
        S = V[:, idx]
        assert len(idx) == len(repeated), (idx, lo, hi)
        for c in repeated:
            out_of = np.linalg.norm(X[:, c] - S @ (S.T @ X[:, c]))
            gap = np.abs(np.delete(lam, idx) - val[c]).min()
            assert out_of <= (res[c] + noise) / gap, "the repeated pair's subspace, vector %d" % c
    return res
