"""Oracle of the linear regression (include/hpgv.h "Linear regression"), written from the definition.

ref_fit() is the reference: ordinary least squares on the UN-CENTRED design [1, d, c ..] in extended precision (np.longdouble),
residuals taken directly; it knows nothing of class sums.  Its tail is scipy.stats.t.sf.

class_sum_fit() is a float64 numpy implementation of the class-sum definition (centred features, G, h, the missing-sample
correction with its selection rule, the back-transformed intercept), forwards and, with reverse=True, with every sum taken in the
opposite order.  Its largest deviation from ref_fit in units of the reference's standard errors, over every case and both
directions, is the rounding yardstick E below.

Also here: the case generator of the tests (cohorts with OTHER columns mixed in, covariates, a trait, HPGV8 rows with missing
calls), the named rows, and what a test may ask of each row (expectations)."""
import functools
import math

import numpy as np
from scipy import stats

from logistic_golden import classify, text_of, format_f6          # the byte rule and the VCF text are the logistic test's

MAX_COVAR = 14
OK, SINGULAR, EXACT = 0, 1, 2
PIVOT_EPS = 1e-12
EXACT_EPS = 1e-12
LD = np.longdouble

# The yardstick: max over all rows expected OK of every case of CASES of |beta - beta_ref| / se_ref and |se - se_ref| / se_ref, every
# coefficient, class_sum_fit in both directions against ref_fit.  Measured on the CPU by measure_E() (tests/test_linear_cpu.py
# asserts that the constant still covers it):
#   measured 2.7e-13 (5 .. 511 cohort samples, C = 0 .. 14, 67 random and 7 or 8 named rows per case, one case with a trait of mean 1000 and
#   sd 10; measured again with the four cases of COVARS_DEAL, C = 8 and 9 at 199 and 511 cohort samples: they reach 3.4e-14 by themselves,
#   the maximum stays where it was)
E = 2.7e-13
# what a host or device result may differ by, in the same units
DEVICE_TOL = max(64 * E, 1e-12)

# hpgv_linear_t_p against 2 * scipy.stats.t.sf over T_GRID_DF x T_GRID_T: the worst relative deviation where scipy's value is at
# least 1e-300, measured on the CPU by measure_tail() (test_linear_cpu.py asserts that the constant still covers it):
#   measured 1.5e-12, at df = 100 000 and t = 2, where x is close to 1 and the fraction's first terms cancel (1e-13 elsewhere)
T_GRID_DF = [1, 2, 3, 5, 10, 30, 100, 1000, 10000, 100000]
T_GRID_T = [0.0, 1e-8, 0.1, 1.0, 2.0, 5.0, 10.0, 40.0, 200.0]
TAIL_DEV = 1.5e-12
P_RTOL = max(1e-10, 4 * TAIL_DEV)

# (nA, nU) of the tests: they move the segment pad, the 16-byte load, the 64-position wave step and the ragged last k-step
SHAPES = [(0, 5), (15, 17), (37, 29), (64, 64), (129, 70), (300, 211)]
COVARS = [0, 1, 3, 13, 14]
N_ROWS = 67                         # random rows per case; the named rows follow them


def tail(t, df):
    """the oracle's two-sided tail"""
    return 2.0 * float(stats.t.sf(abs(float(t)), int(df)))


def _chol_solve(M):
    """(singular, inverse, smallest pivot ratio) of a symmetric matrix in its own precision: right-looking Cholesky without
    pivoting, a pivot <= PIVOT_EPS * M_kk (or NaN) is singular"""
    p = M.shape[0]
    A = M.copy()
    L = np.zeros_like(M)
    ratio = math.inf
    for k in range(p):
        d = A[k, k]
        if not d > PIVOT_EPS * M[k, k]:
            return True, None, 0.0
        ratio = min(ratio, float(d / M[k, k]))
        L[k, k] = np.sqrt(d)
        L[k + 1:, k] = A[k + 1:, k] / L[k, k]
        A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    X = np.zeros_like(M)
    for j in range(p):
        for i in range(j, p):
            s = (1 if i == j else 0) - L[i, j:i] @ X[j:i, j]
            X[i, j] = s / L[i, i]
    return False, X.T @ X, ratio


def _result(n_obs, p, status, beta=None, se=None, ratio=0.0):
    res = dict(n_obs=n_obs, df=n_obs - p, status=status, ratio=ratio, p_dim=p)
    nan = np.full(p, np.nan)
    if status == OK:
        stat = float(beta[1] / se[1])
        res.update(beta=float(beta[1]), se=float(se[1]), stat=stat, p=tail(stat, n_obs - p), coef_beta=beta.astype(np.float64), coef_se=se.astype(np.float64))
    elif status == EXACT:
        res.update(beta=float(beta[1]), se=0.0, stat=np.nan, p=np.nan, coef_beta=beta.astype(np.float64), coef_se=np.zeros(p))
    else:
        res.update(beta=np.nan, se=np.nan, stat=np.nan, p=np.nan, coef_beta=nan, coef_se=nan)
    return res


def ref_fit(cls, y, cov=None):
    """the reference: un-centred design, extended precision, residuals taken directly"""
    cls = np.asarray(cls)
    obs = np.flatnonzero(cls <= 2)
    C = 0 if cov is None else np.asarray(cov).reshape(len(cls), -1).shape[1]
    p = C + 2
    n_obs = len(obs)
    if n_obs - p < 1:
        return _result(n_obs, p, SINGULAR)
    X = np.ones((n_obs, p), LD)
    X[:, 1] = cls[obs]
    if C:
        X[:, 2:] = np.asarray(cov, np.float64).reshape(len(cls), -1)[obs]
    yy = np.asarray(y, np.float64)[obs].astype(LD)
    sing, V, ratio = _chol_solve(X.T @ X)
    if sing:
        return _result(n_obs, p, SINGULAR)
    beta = V @ (X.T @ yy)
    beta = beta + V @ (X.T @ (yy - X @ beta))              # one step of refinement
    r = yy - X @ beta
    rss = r @ r
    yc = yy - yy.mean()
    if rss <= LD(EXACT_EPS) * (yc @ yc):
        return _result(n_obs, p, EXACT, beta, ratio=ratio)
    se = np.sqrt(rss / (n_obs - p) * np.diag(V))
    return _result(n_obs, p, OK, beta, se, ratio)


def class_sum_fit(cls, y, cov=None, reverse=False):
    """the class-sum definition in float64; the samples are the cohort in layout (here: index) order; reverse: every sum over
    samples in the opposite order"""
    cls = np.asarray(cls)
    n = len(cls)
    C = 0 if cov is None else np.asarray(cov).reshape(n, -1).shape[1]
    p = q = C + 2
    order = np.arange(n)[::-1] if reverse else np.arange(n)
    cv = np.zeros((n, 0)) if C == 0 else np.asarray(cov, np.float64).reshape(n, -1)
    yy = np.asarray(y, np.float64)
    raw = np.column_stack([cv, yy])[order]
    c = cls[order]
    mean = raw.sum(axis=0) / max(n, 1)
    F = np.column_stack([np.ones(n), raw - mean])           # [1, c - m, y - m_y]
    G = F.T @ F
    obs = c <= 2
    d = np.where(obs, c, 0).astype(np.float64)
    h = F.T @ d
    n1, n2 = int((c == 1).sum()), int((c == 2).sum())
    n_obs = int(obs.sum())
    n_miss = n - n_obs
    S = G - F[~obs].T @ F[~obs] if n_miss <= n_obs else F[obs].T @ F[obs]
    if n_obs - p < 1:
        return _result(n_obs, p, SINGULAR)
    A = np.zeros((p, p))
    f_of = [0] + [None] + list(range(1, C + 1))              # coefficient -> feature
    iy = q - 1
    b = np.zeros(p)
    for i in range(p):
        for j in range(p):
            if i == 1 and j == 1:
                A[i, j] = n1 + 4 * n2
            elif i == 1 or j == 1:
                o = j if i == 1 else i
                A[i, j] = n1 + 2 * n2 if o == 0 else h[f_of[o]]
            else:
                A[i, j] = S[f_of[i], f_of[j]]
        b[i] = h[iy] if i == 1 else S[f_of[i], iy]
    sing, V, ratio = _chol_solve(A)
    if sing:
        return _result(n_obs, p, SINGULAR)
    Lc = np.linalg.cholesky(A)
    z = np.linalg.solve(Lc, b)
    rss = S[iy, iy] - z @ z
    beta = V @ b
    a = np.concatenate([[1.0, 0.0], -mean[:C]])
    beta0 = beta[0] + mean[C] - beta[2:] @ mean[:C]
    full = beta.copy()
    full[0] = beta0
    if rss <= EXACT_EPS * S[iy, iy]:
        return _result(n_obs, p, EXACT, full, ratio=ratio)
    s2 = rss / (n_obs - p)
    se = np.sqrt(s2 * np.diag(V))
    se[0] = math.sqrt(s2 * (a @ V @ a))
    return _result(n_obs, p, OK, full, se, ratio)


# ---- cases --------------------------------------------------------------------------------------------------------------------

def named_rows(C):
    return (["all_missing", "monomorphic"] + (["collinear_with_covariate"] if C else []) + ["few_obs", "mostly_missing", "no_missing"]
            + (["exact"] if C == 0 else []) + ["byte_codes"])


def make_case(nA, nU, C, trait="unit"):
    """a cohort of nA affected and nU unaffected columns with OTHER columns mixed in, C covariates and a trait (NaN in the OTHER
    columns), and N_ROWS random rows (about 5 % missing) followed by named_rows(C).  The first covariate takes the values -1, 0, 1,
    so that a row can be collinear with it.  trait "mean1000": mean 1000, sd 10.  Returns a dict: cond, cov, y, gt (rows,
    n_samples) HPGV8."""
    rng = np.random.default_rng(7000 * nA + 13 * nU + C + (99 if trait != "unit" else 0))
    n_other = max(2, (nA + nU) // 9)
    cond = np.array([1] * nA + [0] * nU + [2] * n_other, np.uint8)
    rng.shuffle(cond)
    n = len(cond)
    cov = rng.standard_normal((n, C))
    if C:
        cov[:, 0] = rng.integers(0, 3, n) - 1.0
    coh = np.flatnonzero(cond != 2)
    codes = np.array([0x00, 0x01, 0x11], np.uint8)
    rows = []
    for v in range(N_ROWS):
        maf = rng.uniform(0.25, 0.5)
        d = rng.binomial(2, maf, n)
        b = codes[d]
        b = np.where((d == 1) & (rng.random(n) < 0.5), 0x10, b).astype(np.uint8)
        b[rng.random(n) < 0.05] = 0xFF
        rows.append(b)
    base = rows[0].copy()
    d0 = np.where(classify(base) == 255, 1, classify(base)).astype(np.float64)
    y = 0.4 * d0 + (cov @ rng.uniform(-0.5, 0.5, C) if C else 0.0) + rng.standard_normal(n)
    if trait == "mean1000":
        y = 1000.0 + 10.0 * (y - y[coh].mean()) / y[coh].std()
    cov[cond == 2] = np.nan
    y[cond == 2] = np.nan
    p = C + 2
    names = named_rows(C)
    for name in names:
        b = base.copy()
        if name == "all_missing":
            b[:] = 0xFF
        elif name == "monomorphic":
            b[classify(b) != 255] = 0x11
        elif name == "collinear_with_covariate":           # d = c_1 + 1 on every observation
            b = np.where(classify(base) == 255, 0xFF, 0).astype(np.uint8)
            keep = (b == 0) & (cond != 2)
            b[keep] = codes[(cov[keep, 0] + 1).astype(int)]
        elif name == "few_obs":                             # n_obs = p (or the whole cohort where it is smaller): df < 1
            b[:] = 0xFF
            keep = coh[:p]
            b[keep] = codes[np.arange(len(keep)) % 3]
        elif name == "mostly_missing":                      # n_miss > n_obs: S is summed over the observed columns
            b[:] = 0xFF
            keep = coh[::3][:max(1, (len(coh) - 1) // 2)]
            b[keep] = codes[rng.integers(0, 3, len(keep))]
        elif name == "no_missing":
            b[classify(b) == 255] = 0x01
        elif name == "exact":                               # the trait of this row's observations is 3 + 2 d: see exact_trait
            b = codes[rng.integers(0, 3, n)]
            b[coh[1::7]] = 0xFF
        elif name == "byte_codes":                          # 1/2 and 2/1 are hom-alt, 2/0 het; a nibble 0xF alone is missing
            strict = np.array([0x12, 0x21, 0x20, 0x02, 0x0F, 0xF0, 0xF1, 0xFF, 0x22, 0x00, 0x01, 0x11, 0x13, 0x30], np.uint8)
            b = strict[rng.integers(0, len(strict), n)]
        rows.append(b)
    gt = np.ascontiguousarray(np.stack(rows))
    case = dict(nA=nA, nU=nU, C=C, trait=trait, cond=cond, cov=cov, y=y, gt=gt, coh=coh, names=names)
    if "exact" in names:                                    # a second trait for that row alone: y = 3 + 2 d where d is observed
        r = N_ROWS + names.index("exact")
        cl = classify(gt[r])
        ye = np.where(cl <= 2, 3.0 + 2.0 * np.minimum(cl, 2), 7.5)
        ye[cond == 2] = np.nan
        case["exact_row"], case["y_exact"] = r, ye
    return case


def cohort_view(case, row, y=None):
    """(cls, y, cov) of a row's cohort columns in VCF column order: what hpgv_linear_fit and the fits above take"""
    coh = case["coh"]
    return classify(case["gt"][row, coh]), (case["y"] if y is None else y)[coh], case["cov"][coh]


# what a test may ask of a row:
#   "ok"        ref_fit gives OK with every pivot ratio above 1e-6: numbers within DEVICE_TOL, P by the tail rule
#   "singular"  singular by construction or df < 1: status SINGULAR, NaN
#   "exact"     the trait is an exact function of the design: status EXACT, beta within DEVICE_TOL of the truth (in units of 1)
#   "loose"     badly conditioned: n_obs and df only, and NaN unless the status is OK or EXACT
@functools.lru_cache(maxsize=None)
def expectations(nA, nU, C, trait="unit"):
    case = make_case(nA, nU, C, trait)
    out = []
    for r in range(len(case["gt"])):
        name = case["names"][r - N_ROWS] if r >= N_ROWS else "random"
        if name == "exact":
            continue
        cls, y, cov = cohort_view(case, r)
        ref = ref_fit(cls, y, cov)
        if name in ("all_missing", "monomorphic", "collinear_with_covariate", "few_obs") or ref["df"] < 1:
            kind = "singular"
        elif ref["status"] == OK and ref["ratio"] > 1e-6:
            kind = "ok"
        else:
            kind = "loose"
        out.append(dict(kind=kind, name=name, row=r, ref=ref))
    return case, out


def well_sized(nA, nU, C, trait="unit"):
    """cases whose random rows must be OK nine times in ten: n_obs >= 4 p with room for the missing calls"""
    return 0.9 * (nA + nU) >= 4 * (C + 2)


def case_id(k):
    return "%dx%d_C%d_%s" % k


# k_linear deals the ne = q (q + 1) / 2 entries of S, q = C + 2, to the 64 lanes of a wave: entry lane + 64 t, t = 0, 1, 2.  COVARS
# gives ne = 3, 6, 15, 120 and 136; COVARS_DEAL stands on either side of the step from one entry per lane to two: C = 8 has ne = 55,
# C = 9 has ne = 66, the lanes 0 and 1 alone with a second entry.
SHAPES_DEAL = [(129, 70), (300, 211)]
COVARS_DEAL = [8, 9]

CASES = ([(nA, nU, C, "unit") for nA, nU in SHAPES for C in COVARS] + [(300, 211, 3, "mean1000")]
         + [(nA, nU, C, "unit") for nA, nU in SHAPES_DEAL for C in COVARS_DEAL])


def measure_E():
    worst = 0.0
    for key in CASES:
        case, exp = expectations(*key)
        for e in exp:
            if e["kind"] != "ok":
                continue
            cls, y, cov = cohort_view(case, e["row"])
            ref = e["ref"]
            for rev in (False, True):
                f = class_sum_fit(cls, y, cov, reverse=rev)
                assert f["status"] == OK, (key, e["row"])
                worst = max(worst, np.max(np.abs(f["coef_beta"] - ref["coef_beta"]) / ref["coef_se"]), np.max(np.abs(f["coef_se"] - ref["coef_se"]) / ref["coef_se"]))
    return worst


def measure_tail(t_p):
    """worst relative deviation of t_p(t, df) from the oracle's tail on the grid, where the oracle's value is at least 1e-300"""
    worst = 0.0
    for df in T_GRID_DF:
        for t in T_GRID_T:
            for sgn in (1.0, -1.0):
                want, got = tail(t, df), t_p(sgn * t, df)
                if want < 1e-300:
                    assert 0.0 <= got <= 1e-299, (t, df, got)
                    continue
                worst = max(worst, abs(got - want) / want)
    return worst


def check_p(got_p, got_stat, df, where=""):
    """P against the oracle's tail at the tested STAT and df"""
    want = tail(got_stat, df)
    if want < 1e-300:
        assert 0.0 <= got_p <= 1e-299, (where, got_p, want)
    else:
        assert abs(got_p - want) <= P_RTOL * want, (where, got_p, want, P_RTOL)


def check_row(rec, coef, e, where=""):
    """one hpgv_linear_result record (and its coef (2, p) or None) against a row's expectation.  Returns the worst deviation in
    units of the reference's standard errors (0 for a row that is not "ok")."""
    ref, tol = e["ref"], DEVICE_TOL
    assert rec["n_obs"] == ref["n_obs"] and rec["df"] == ref["df"] and rec["pad"] == 0, (where, rec, ref["n_obs"])
    all_nan = all(np.isnan(rec[k]) for k in ("beta", "se", "stat", "p")) and (coef is None or np.all(np.isnan(coef)))
    if e["kind"] == "ok":
        assert rec["status"] == OK, (where, rec["status"])
        eb, es = abs(rec["beta"] - ref["beta"]) / ref["se"], abs(rec["se"] - ref["se"]) / ref["se"]
        assert eb <= tol and es <= tol, (where, eb, es, tol)
        # stat = beta / se with |d beta| and |d se| <= tol se: |d stat| <= tol (1 + |stat|) / (1 - tol)
        assert abs(rec["stat"] - ref["stat"]) <= 1.01 * tol * (1.0 + abs(ref["stat"])), (where, rec["stat"], ref["stat"])
        check_p(rec["p"], rec["stat"], rec["df"], where)
        worst = max(eb, es)
        if coef is not None:
            db, ds = np.abs(coef[0] - ref["coef_beta"]) / ref["coef_se"], np.abs(coef[1] - ref["coef_se"]) / ref["coef_se"]
            assert np.all(db <= tol) and np.all(ds <= tol), (where, db.max(), ds.max(), tol)
            assert coef[0][1] == rec["beta"] and coef[1][1] == rec["se"], where
            worst = max(worst, db.max(), ds.max())
        return worst
    if e["kind"] == "singular":
        assert rec["status"] == SINGULAR and all_nan, (where, rec["status"])
    else:
        assert rec["status"] in (OK, SINGULAR, EXACT) and (rec["status"] != SINGULAR or all_nan), (where, rec["status"])
    return 0.0


def check_exact(rec, coef, where=""):
    """the row whose trait is 3 + 2 d, at C = 0"""
    assert rec["status"] == EXACT and rec["se"] == 0.0 and np.isnan(rec["stat"]) and np.isnan(rec["p"]), (where, rec)
    assert abs(rec["beta"] - 2.0) <= DEVICE_TOL, (where, rec["beta"])
    if coef is not None:
        assert abs(coef[0][0] - 3.0) <= DEVICE_TOL and coef[0][1] == rec["beta"] and np.all(coef[1] == 0.0), (where, coef)


def format_line(chrom, pos, vid, ref, alt, r):
    """the runner's line for an oracle (or device) result r: a dict or record with n_obs, beta, se, stat, p"""
    return "\t".join([chrom, str(pos), vid, ref, alt, str(int(r["n_obs"]))] + [format_f6(float(r[k])) for k in ("beta", "se", "stat", "p")])
