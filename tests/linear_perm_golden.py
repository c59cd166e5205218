"""Oracle of the permutations of the linear statistic (include/hpgv.h "permutations of the linear statistic"), written from the
definition's meaning.

oracle() is the reference: for every row and permutation an ordinary least squares fit, by the normal equations in extended
precision (np.longdouble), of the Freedman-Lane trait y*_p = Z gamma + eps_p on the design [Z, g] -- Z = [1, c_1 .. c_C], g the
row's dosage with its missing calls set to the mean of the observed ones -- and the t statistic of g with df = N - p.  It knows
nothing of the orthonormal basis Q or of the r2 form.  Whether a row takes part it decides from the same fit: D is the Schur
complement of g in [Z, g]^T [Z, g].

closed_form() is a float64 numpy implementation of the definition as the header states it (Q by modified Gram-Schmidt, e, E_p,
ss_p, then mu, D, u and r2 per row).  Its largest deviation from oracle(), in t units relative to max(1, |T|), over every case is
the rounding yardstick E_PERM below.

Also here: the cases (the cohorts, covariates and traits of linear_golden.make_case, rows of their own with 0 %, 2 % and 60 %
missing calls and the named rows), the permutations (numpy's generator: the oracle does not depend on the library's shuffle), a
Python transcription of the documented shuffle, and the counts a test may ask for.

# E_PERM: measured 8.8e-14 on the CPU by measure_E() over CASES, at the cohort of 5 columns with one covariate (df = 2); the cohorts of
# 32 to 4 100 columns stay below 3.3e-14, the trait of mean 1000 being the worst (test_linear_perm_cpu.py asserts that the constant
# still covers it).
# The largest deviation of the device from the oracle observed on an MI355X over the cases of test_linear_perm_gpu.py: 3.7e-14, at the
# trait of mean 1000 (2.1e-14 at 4 100 cohort columns, below 7e-15 elsewhere): DEVICE_SEEN below."""
import functools

import numpy as np

import linear_golden as ln
from linear_golden import LD, classify, text_of, format_f6          # noqa: F401  (the tests take them from here)

EPS = 1e-12
N_PERMS = 257                        # per case; a test with fewer takes the first ones
N_ROWS = ln.N_ROWS                   # random rows per case: a third each with 0 %, 2 % and 60 % missing calls
MISSING = (0.0, 0.02, 0.6)

E_PERM = 8.8e-14
HOST_TOL = max(4 * E_PERM, 1e-12)
DEVICE_TOL = max(64 * E_PERM, 1e-12)
DEVICE_SEEN = 3.7e-14                # measured on an MI355X; a record, no test reads it

# (nA, nU, C, trait).  (0, 5): the no-part rules only (df < 1 from C = 3 on; no counts are asked of a cohort below 17 columns)
LONG = (2100, 2000)
CASES = ([(nA, nU, C, "unit") for nA, nU in ln.SHAPES for C in ln.COVARS if (nA, nU) != (0, 5) or C <= 3]
         + [LONG + (3, "unit"), (300, 211, 3, "mean1000")])
COUNT_CASES = [k for k in CASES if k[0] + k[1] >= 17]


def case_id(k):
    return "%dx%d_C%d_%s" % k


def named_rows(C):
    return (["all_missing", "monomorphic", "single_het", "one_observation"] + (["equals_covariate"] if C else [])
            + ["missing_gt_observed", "missing_last_of_segments"])


@functools.lru_cache(maxsize=None)
def make_case(nA, nU, C, trait="unit"):
    """cond, cov, y, coh of linear_golden.make_case; gt: N_ROWS random rows, then named_rows(C); order (N_PERMS, n_samples) int32:
    row p column j = the column whose residual column j takes, OTHER columns fixed, no row the identity"""
    base = ln.make_case(nA, nU, C, trait)
    cond, cov, coh = base["cond"], base["cov"], base["coh"]
    n = len(cond)
    rng = np.random.default_rng(991 * nA + 17 * nU + 3 * C + (5 if trait != "unit" else 0) + 1)
    codes = np.array([0x00, 0x01, 0x11], np.uint8)
    rows = []
    for v in range(N_ROWS):
        maf = rng.uniform(0.1, 0.5)
        d = rng.binomial(2, maf, n)
        b = np.where((d == 1) & (rng.random(n) < 0.5), 0x10, codes[d]).astype(np.uint8)
        b[rng.random(n) < MISSING[v % 3]] = 0xFF
        rows.append(b)
    full = codes[rng.binomial(2, 0.3, n)]
    names = named_rows(C)
    for name in names:
        b = full.copy()
        if name == "all_missing":
            b[:] = 0xFF
        elif name == "monomorphic":
            b[:] = 0x11
            b[coh[::5]] = 0xFF
        elif name == "single_het":
            b[:] = 0x00
            b[coh[len(coh) // 2]] = 0x10
            b[coh[1::6]] = 0xFF
        elif name == "one_observation":
            b[:] = 0xFF
            b[coh[len(coh) // 3]] = 0x01
        elif name == "equals_covariate":                    # d = c_1 + 1 on every cohort column, none missing
            b[coh] = codes[(cov[coh, 0] + 1).astype(int)]
        elif name == "missing_gt_observed":                 # three calls in five missing, every class among the rest
            b[coh] = codes[rng.permutation(len(coh)) % 3]
            b[coh[np.arange(len(coh)) % 5 < 3]] = 0xFF
        elif name == "missing_last_of_segments":            # the last affected and the last unaffected column
            for c in (1, 0):
                seg = np.flatnonzero(cond == c)
                if len(seg):
                    b[seg[-1]] = 0xFF
        rows.append(b)
    order = np.tile(np.arange(n, dtype=np.int32), (N_PERMS, 1))
    for p in range(N_PERMS):
        while True:
            sh = rng.permutation(coh)
            if len(coh) < 2 or np.any(sh != coh):
                break
        order[p, coh] = sh
    return dict(nA=nA, nU=nU, C=C, trait=trait, cond=cond, cov=cov, y=base["y"], coh=coh, names=names, gt=np.ascontiguousarray(np.stack(rows)),
                order=order)


def cohort_view(case):
    """(cls (rows, N), y (N,), cov (N, C), order (N_PERMS, N) as indices into the cohort) in VCF column order of the cohort: what
    hpgv_linear_perm_fit, oracle() and closed_form() take"""
    coh = case["coh"]
    idx = np.full(len(case["cond"]), -1, np.int64)
    idx[coh] = np.arange(len(coh))
    return classify(case["gt"][:, coh]), case["y"][coh], case["cov"][coh], idx[case["order"][:, coh]].astype(np.int32)


def _imputed(cls_row, dtype):
    obs = cls_row <= 2
    n_obs = int(obs.sum())
    if n_obs == 0:
        return None, obs, 0
    d = np.where(obs, cls_row, 0).astype(dtype)
    mu = d.sum() / dtype(n_obs)
    return np.where(obs, d, mu), obs, n_obs


def oracle(cls, y, cov, order):
    """(t_obs (rows,), T (rows, P), ratio (rows,)): extended precision; NaN where the definition says so.  ratio = D / sw2 of the
    rows with observations and a spread (else 0): a test asserts that no row lies near the rule's 1e-12"""
    cls = np.asarray(cls)
    R, N = cls.shape
    C = 0 if cov is None else np.asarray(cov).reshape(N, -1).shape[1]
    p, P = C + 2, len(order)
    df = N - p
    t_obs, T, ratio = np.full(R, np.nan), np.full((R, P), np.nan), np.zeros(R)
    if df < 1:
        return t_obs, T, ratio
    Z = np.ones((N, C + 1), LD)
    if C:
        Z[:, 1:] = np.asarray(cov, np.float64).reshape(N, -1)
    yy = np.asarray(y, np.float64).astype(LD)
    sing, Vz, _ = ln._chol_solve(Z.T @ Z)
    assert not sing
    gamma = Vz @ (Z.T @ yy)
    gamma = gamma + Vz @ (Z.T @ (yy - Z @ gamma))
    fitted = Z @ gamma
    e = yy - fitted
    Y = np.empty((N, P + 1), LD)                            # column 0: the trait itself, then y*_p
    Y[:, 0] = yy
    Y[:, 1:] = fitted[:, None] + e[np.asarray(order).T]
    ZtZ, ZtY, yty = Z.T @ Z, Z.T @ Y, np.einsum("ij,ij->j", Y, Y)
    for r in range(R):
        g, obs, n_obs = _imputed(cls[r], LD)
        if n_obs == 0:
            continue
        w = np.where(obs, g - g[obs].sum() / LD(n_obs), LD(0))
        sw2 = w @ w
        if not sw2 > 0:
            continue
        Ztg = Z.T @ g
        D = g @ g - Ztg @ (Vz @ Ztg)
        ratio[r] = float(D / sw2)
        if not D > LD(EPS) * sw2:
            continue
        A = np.empty((p, p), LD)
        A[:p - 1, :p - 1], A[:p - 1, p - 1], A[p - 1, :p - 1], A[p - 1, p - 1] = ZtZ, Ztg, Ztg, g @ g
        sing, V, _ = ln._chol_solve(A)
        assert not sing, r
        b = np.vstack([ZtY, (g @ Y)[None, :]])
        beta = V @ b
        rss = yty - np.einsum("ij,ij->j", b, beta)
        t = beta[p - 1] / np.sqrt(rss / LD(df) * V[p - 1, p - 1])
        r2 = t * t / (LD(df) + t * t)
        t = np.where(r2 < 1 - LD(EPS), t, np.nan).astype(np.float64)
        t_obs[r], T[r] = t[0], t[1:]
    return t_obs, T, ratio


def closed_form(cls, y, cov, order):
    """(t_obs, T) by the header's closed form in float64"""
    cls = np.asarray(cls)
    R, N = cls.shape
    C = 0 if cov is None else np.asarray(cov).reshape(N, -1).shape[1]
    p, P = C + 2, len(order)
    df = N - p
    cv = np.zeros((N, 0)) if C == 0 else np.asarray(cov, np.float64).reshape(N, -1)
    Q = np.zeros((N, C))

    def project(v):
        for k in range(C):
            v = v - Q[:, k] * (Q[:, k] @ v)
        return v
    for k in range(C):
        v = cv[:, k] - cv[:, k].sum() / N
        n0 = v @ v
        for j in range(k):
            v = v - Q[:, j] * (Q[:, j] @ v)
        rem = v @ v
        assert rem > EPS * n0
        Q[:, k] = v / np.sqrt(rem)
    yy = np.asarray(y, np.float64)
    e = project(yy - yy.sum() / N)
    E = np.empty((N, P + 1))
    E[:, 0] = e
    for q in range(P):
        eps = e[order[q]]
        E[:, q + 1] = project(eps - eps.sum() / N)
    ss = np.einsum("ij,ij->j", E, E)
    t_obs, T = np.full(R, np.nan), np.full((R, P), np.nan)
    for r in range(R):
        obs = cls[r] <= 2
        n_obs, n1, n2 = int(obs.sum()), int((cls[r] == 1).sum()), int((cls[r] == 2).sum())
        if n_obs == 0 or df < 1:
            continue
        mu = (n1 + 2 * n2) / n_obs
        sw2 = (n1 + 4 * n2) - n_obs * mu * mu
        if not sw2 > 0:
            continue
        d = np.where(obs, cls[r], 0).astype(np.float64)
        v = obs.astype(np.float64)
        gq = d @ Q - mu * (v @ Q)
        D = sw2 - gq @ gq
        if not D > EPS * sw2:
            continue
        u = d @ E - mu * (v @ E)
        with np.errstate(invalid="ignore", divide="ignore"):
            r2 = u * u / (D * ss)
            t = np.where(r2 < 1 - EPS, np.sign(u) * np.sqrt(df * r2 / (1 - r2)), np.nan)
        t_obs[r], T[r] = t[0], t[1:]
    return t_obs, T


def deviation(got, want):
    """the largest |got - want| / max(1, |want|); inf where one is NaN and the other is not"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if np.any(np.isnan(got) != np.isnan(want)):
        return np.inf
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))))


@functools.lru_cache(maxsize=None)
def expectations(nA, nU, C, trait="unit"):
    """(case, dict(t_obs, T, ratio, part)) of a case: the oracle over all rows and N_PERMS permutations"""
    case = make_case(nA, nU, C, trait)
    cls, y, cov, order = cohort_view(case)
    t_obs, T, ratio = oracle(cls, y, cov, order)
    for a in (t_obs, T, ratio):
        a.setflags(write=False)
    N, p = nA + nU, C + 2
    part = (ratio > EPS) & (N - p >= 1)
    return case, dict(t_obs=t_obs, T=T, ratio=ratio, part=part)


def counts(exp, rows=slice(None), n_perms=N_PERMS, tol=DEVICE_TOL):
    """what the oracle says of the rows `rows` under the first n_perms permutations: n_ge per row and batch_max per permutation,
    with the number of undecided pairs -- ||T_p| - |T_obs|| within 2 tol max(1, |T|) -- and of undecided (row, maximum) pairs"""
    t_obs, T, part = np.abs(exp["t_obs"][rows]), np.abs(exp["T"][rows, :n_perms]), exp["part"][rows]
    with np.errstate(invalid="ignore"):
        ge = T >= t_obs[:, None]                             # False where either is NaN
        scale = np.maximum(1.0, np.maximum(T, t_obs[:, None]))
        und = np.abs(T - t_obs[:, None]) <= 2 * tol * scale
        Tm = np.where(np.isnan(T) | ~part[:, None], 0.0, T)
        bmax = Tm.max(axis=0) if len(Tm) else np.zeros(n_perms)
        und_max = np.abs(bmax[None, :] - t_obs[:, None]) <= 2 * tol * np.maximum(1.0, np.maximum(bmax[None, :], t_obs[:, None]))
    return dict(n_ge=ge.sum(axis=1).astype(np.int32), batch_max=bmax, undecided=int(und.sum()), undecided_max=int(und_max.sum()))


def measure_E():
    worst = 0.0
    for key in CASES:
        case, exp = expectations(*key)
        t_obs, T = closed_form(*cohort_view(case))
        worst = max(worst, deviation(t_obs, exp["t_obs"]), deviation(T, exp["T"]))
    return worst


# ---- the documented shuffle -----------------------------------------------------------------------------------------------------

M64 = (1 << 64) - 1


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def order_shuffle(cond, n_perms, seed):
    """hpgv_perm_order_shuffle as include/hpgv.h documents it: key = SplitMix64(seed ^ SplitMix64(p)), draw i = SplitMix64(key + i),
    Fisher-Yates from the last cohort column down, j = the high 64 bits of draw x i"""
    cond = np.asarray(cond)
    cols = [j for j in range(len(cond)) if cond[j] in (0, 1)]
    out = np.tile(np.arange(len(cond), dtype=np.int32), (n_perms, 1))
    for p in range(n_perms):
        y = list(cols)
        key = splitmix64((seed & M64) ^ splitmix64(p))
        draw = 0
        for i in range(len(y), 1, -1):
            r = splitmix64((key + draw) & M64)
            draw += 1
            j = (r * i) >> 64
            y[i - 1], y[j] = y[j], y[i - 1]
        for k, c in enumerate(cols):
            out[p, c] = y[k]
    return out
