"""Oracle of the logistic regression (include/hpgv.h "Logistic regression"), in plain numpy f64, written from the definition: the
byte rule, the observations, Newton-Raphson from beta = 0 with a Cholesky step and the pivot rule, V of the last step's H, the
status rules.  It sums the samples by matrix products -- forwards and, with reverse=True, in the opposite order; the largest
difference between the two over every generated case is the rounding yardstick E below.

Also here: the case generator of the tests (cohorts with OTHER columns mixed in, covariates, HPGV8 rows with missing calls), the
status rows, and what a test may ask of each row (expectations)."""
import functools
import math

import numpy as np

MAX_COVAR = 14
OK, NOT_CONVERGED, SINGULAR = 0, 1, 2
PIVOT_EPS = 1e-12
MAX_ITER, TOL = 25, 1e-10          # the runner's, and the tests'

# The yardstick: max over all rows expected OK of every case of CASES and of the nested cases of |beta_fwd - beta_rev| / se and
# |se_fwd - se_rev| / se, every coefficient.  Measured on the CPU by measure_E() (tests/test_logistic_cpu.py asserts that the constant still covers it):
#   measured 7.0e-14 (32 .. 1300 cohort samples, C = 0 .. 14, 67 + 8 rows per case of CASES and the 67 rows of the four nested
#   cases; 5.2e-14 over SHAPES x COVARS alone, 70 .. 530 samples)
E = 7.0e-14
# what a device result may differ by, in the same units: another summation tree, fma, another exp
DEVICE_TOL = max(64 * E, 1e-12)

# (nA, nU) of the GPU tests: pads inside and at the end of both segments, one lane step and several, a ragged last step
SHAPES = [(1, 1), (15, 17), (37, 29), (64, 64), (129, 70), (300, 211)]
COVARS = [0, 1, 3, 13, 14]
N_ROWS = 67                         # random rows per case; the status rows follow them


def classify(b):
    """genotype class of HPGV8 bytes: 0 / 1 / 2, 255 = missing"""
    b = np.asarray(b, np.uint8)
    lo, hi = b & 15, b >> 4
    cls = ((lo != 0).astype(np.uint8) + (hi != 0).astype(np.uint8))
    return np.where((lo == 15) | (hi == 15), 255, cls).astype(np.uint8)


def chol_inv(H):
    """(singular, V, smallest pivot ratio): right-looking Cholesky without pivoting, a pivot <= PIVOT_EPS * H_kk (or NaN) is
    singular; V = L^-T L^-1"""
    p = H.shape[0]
    A = H.copy()
    L = np.zeros_like(H)
    ratio = math.inf
    for k in range(p):
        d = A[k, k]
        if not d > PIVOT_EPS * H[k, k]:
            return True, None, 0.0
        ratio = min(ratio, d / H[k, k])
        L[k, k] = math.sqrt(d)
        L[k + 1:, k] = A[k + 1:, k] / L[k, k]
        A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    X = np.zeros_like(H)
    for j in range(p):
        for i in range(j, p):
            s = (1.0 if i == j else 0.0) - L[i, j:i] @ X[j:i, j]
            X[i, j] = s / L[i, i]
    return False, X.T @ X, ratio


def chisq_p(x):
    """the 1-df chi-square tail as hpgv_assoc_chisq_dev's device function writes it"""
    if x != x:
        return x
    if x <= 0.0:
        return 1.0
    y = x / 2.0
    P = 1.0 - math.erfc(math.sqrt(y)) if y > 0.5 else math.erf(math.sqrt(y))
    return 1.0 - P


def fit(cls, y, cov=None, max_iter=MAX_ITER, tol=TOL, reverse=False):
    """the definition on samples in index order (reverse: in the opposite order).  cls: 0 / 1 / 2, anything else missing."""
    cls = np.asarray(cls)
    obs = np.flatnonzero(cls <= 2)
    if reverse:
        obs = obs[::-1]
    C = 0 if cov is None else np.asarray(cov).reshape(len(cls), -1).shape[1]
    p = C + 2
    X = np.ones((len(obs), p))
    X[:, 1] = cls[obs]
    if C:
        X[:, 2:] = np.asarray(cov, np.float64).reshape(len(cls), -1)[obs]
    yy = np.asarray(y, np.float64)[obs]
    beta = np.zeros(p)
    status, iters, converged, V, ratio = OK, 0, False, None, math.inf
    for _ in range(max_iter):
        eta = X @ beta
        with np.errstate(over="ignore"):
            mu = 1.0 / (1.0 + np.exp(-eta))
        w = mu * (1.0 - mu)
        H = (X * w[:, None]).T @ X
        u = X.T @ (yy - mu)
        sing, V, r = chol_inv(H)
        if sing:
            status = SINGULAR
            break
        ratio = min(ratio, r)
        delta = V @ u
        beta = beta + delta
        iters += 1
        if not np.all(np.isfinite(beta)):
            status = NOT_CONVERGED
            break
        if np.max(np.abs(delta)) <= tol:
            converged = True
            break
    if not converged and status == OK:
        status = NOT_CONVERGED
    res = dict(n_obs=len(obs), iters=iters, status=status, ratio=ratio, p_dim=p)
    if status == OK:
        se = np.sqrt(np.diag(V))
        stat = (beta[1] / se[1]) ** 2
        res.update(beta=beta[1], se=se[1], stat=stat, p=chisq_p(stat), coef_beta=beta, coef_se=se)
    else:
        nan = np.full(p, np.nan)
        res.update(beta=np.nan, se=np.nan, stat=np.nan, p=np.nan, coef_beta=nan, coef_se=nan)
    return res


# ---- cases --------------------------------------------------------------------------------------------------------------------

STATUS_ROWS = ["all_missing", "monomorphic", "monomorphic_alt", "single_het", "few_obs", "one_class", "separated", "byte_codes"]


def make_case(nA, nU, C, seed=None):
    """a cohort of nA affected and nU unaffected columns with OTHER columns mixed in, C covariates (NaN in the OTHER columns), and
    N_ROWS random rows (about 5 % missing) followed by the STATUS_ROWS.  Returns a dict: cond, cov, gt (rows, n_samples) HPGV8."""
    rng = np.random.default_rng(1000 * nA + 10 * nU + C if seed is None else seed)
    n_other = max(2, (nA + nU) // 9)
    cond = np.array([1] * nA + [0] * nU + [2] * n_other, np.uint8)
    rng.shuffle(cond)
    n = len(cond)
    cov = rng.standard_normal((n, C))
    cov[cond == 2] = np.nan
    aff, una = np.flatnonzero(cond == 1), np.flatnonzero(cond == 0)
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
    p = C + 2
    for name in STATUS_ROWS:
        b = base.copy()
        if name == "all_missing":
            b[:] = 0xFF
        elif name == "monomorphic":
            b[classify(b) != 255] = 0x00
        elif name == "monomorphic_alt":
            b[classify(b) != 255] = 0x11
        elif name == "single_het":
            b[:] = 0x00
            b[aff[0]] = 0x01
        elif name == "few_obs":                 # p - 1 observations
            b[:] = 0xFF
            keep = coh[:p - 1]
            b[keep] = base[keep]
            b[keep[classify(base[keep]) == 255]] = 0x01
        elif name == "one_class":
            b[una] = 0xFF
        elif name == "separated":
            b[aff] = 0x11
            b[una] = 0x00
        elif name == "byte_codes":              # 1/2 and 2/1 are hom-alt, 2/0 het; a nibble 0xF alone is missing
            strict = np.array([0x12, 0x21, 0x20, 0x02, 0x0F, 0xF0, 0xF1, 0xFF, 0x22, 0x00, 0x01, 0x11, 0x13, 0x30], np.uint8)
            b = strict[rng.integers(0, len(strict), n)]
        rows.append(b)
    return dict(nA=nA, nU=nU, C=C, cond=cond, cov=cov, gt=np.ascontiguousarray(np.stack(rows)), aff=aff, una=una, coh=coh)


def cohort_view(case, row):
    """(cls, y, cov) of a row's cohort columns in VCF column order: what hpgv_logistic_fit and fit() take"""
    coh = case["coh"]
    return classify(case["gt"][row, coh]), (case["cond"][coh] == 1).astype(np.uint8), case["cov"][coh]


# what a test may ask of a row:
#   "ok"        fit() gives OK in both orders with every pivot ratio above 1e-6 within 12 steps: numbers within DEVICE_TOL
#   "singular"  singular by construction: status SINGULAR, NaN
#   "nan"       separated or close to it (not OK in some order): NaN with status NOT_CONVERGED or SINGULAR
#   "loose"     converges, but slowly or badly conditioned: n_obs only, and NaN unless the status is OK
def _expect_rows(case, rows):
    C = case["C"]
    out = []
    for r in rows:
        cls, y, cov = cohort_view(case, r)
        f, b = fit(cls, y, cov), fit(cls, y, cov, reverse=True)
        name = STATUS_ROWS[r - N_ROWS] if r >= N_ROWS else "random"
        n_obs, p = f["n_obs"], C + 2
        by_construction = name in ("all_missing", "monomorphic", "monomorphic_alt", "few_obs") or n_obs < p
        if by_construction:
            kind = "singular"
        elif f["status"] == OK and b["status"] == OK and min(f["ratio"], b["ratio"]) > 1e-6 and max(f["iters"], b["iters"]) <= 12:
            kind = "ok"
        elif f["status"] != OK and b["status"] != OK:
            kind = "nan"
        else:
            kind = "loose"
        out.append(dict(kind=kind, name=name, fwd=f, rev=b))
    return out


@functools.lru_cache(maxsize=None)
def expectations(nA, nU, C):
    case = make_case(nA, nU, C)
    return case, _expect_rows(case, range(len(case["gt"])))


@functools.lru_cache(maxsize=None)
def nested_expectations(C):
    """the random rows of the NESTED cohort with the first C of its covariate columns: the same cohort, the same rows and nested
    designs at every C, so that two neighbouring C differ in the kernel that runs them and in one column.  (The status rows are built
    for the widest design and stay out.)"""
    nA, nU, widest = NESTED
    assert C <= widest
    full = make_case(nA, nU, widest)
    case = dict(full, C=C, cov=np.ascontiguousarray(full["cov"][:, :C]), gt=np.ascontiguousarray(full["gt"][:N_ROWS]))
    return case, _expect_rows(case, range(N_ROWS))


def well_sized(nA, nU, C):
    """cases whose random rows must be OK nine times in ten: at least 12 cohort samples per coefficient"""
    return nA + nU >= 12 * (C + 2)


# k_logistic<P, DEAL> by p = C + 2 (logistic_launch), and the zero pad coordinates P - p:
#   C = 0         <2, 1>   pad 0            C = 5, 6      <8, 1>   pad 1, 0
#   C = 1, 2      <4, 1>   pad 1, 0         C = 7 .. 10   <12, 2>  pad 3, 2, 1, 0
#   C = 3, 4      <6, 1>   pad 1, 0         C = 11 .. 14  <16, 4>  pad 3, 2, 1, 0
# COVARS reaches <2,1>, <4,1>, <6,1> and <16,4> with pads 0 and 1; COVARS_MORE the other two kernels, every P filled exactly
# (C = 2, 4, 6, 10) and three pad coordinates (C = 7).  (15, 17) is small for these p: its status rows stay honest, its random rows
# are mostly "loose"; the two larger shapes are well_sized at every C of COVARS_MORE.
SHAPES_MORE = [(15, 17), (129, 70), (300, 211)]
COVARS_MORE = [2, 4, 5, 6, 7, 9, 10]
# One long cohort: a pitch above 1024 positions.  A lane's sample loop advances 512 positions per turn with DEAL = 1, 256 with
# DEAL = 2 and 128 with DEAL = 4, so the waves take 2 or 3 (C = 3: <6,1>, C = 6: <8,1>), 5 or 6 (C = 10: <12,2>) and 10 or 11
# (C = 14: <16,4>) turns, and the last turn is ragged in each.
LONG = (700, 600)
COVARS_LONG = [3, 6, 10, 14]
# The dispatch edges: one cohort, the same rows, the first C columns of one covariate matrix -- <8,1> | <12,2> between C = 6 and 7,
# <12,2> | <16,4> between C = 10 and 11 (nested_expectations)
NESTED = (129, 70, 11)
COVARS_NESTED = [6, 7, 10, 11]

CASES = ([(nA, nU, C) for nA, nU in SHAPES for C in COVARS] + [(nA, nU, C) for nA, nU in SHAPES_MORE for C in COVARS_MORE]
         + [LONG + (C,) for C in COVARS_LONG])


def measure_E():
    worst = 0.0
    for exp in [expectations(*key)[1] for key in CASES] + [nested_expectations(C)[1] for C in COVARS_NESTED]:
        for e in exp:
            if e["kind"] != "ok":
                continue
            f, b = e["fwd"], e["rev"]
            worst = max(worst, np.max(np.abs(f["coef_beta"] - b["coef_beta"]) / f["coef_se"]), np.max(np.abs(f["coef_se"] - b["coef_se"]) / f["coef_se"]))
    return worst


def check_numbers(got_beta, got_se, got_stat, got_p, got_iters, ref, where=""):
    """a device / host result of a row expected "ok" against the oracle, by the issue's tolerances.  Returns the figures."""
    tol = DEVICE_TOL
    eb, es = abs(got_beta - ref["beta"]) / ref["se"], abs(got_se - ref["se"]) / ref["se"]
    assert eb <= tol and es <= tol, (where, eb, es, tol)
    # stat = (beta / se)^2: d stat / stat = 2 (d beta / beta - d se / se), with |d beta| and |d se| <= tol * se
    z = abs(ref["beta"]) / ref["se"]
    rel_stat = 2.0 * (tol / z + tol) if z > 0 else math.inf
    if z > 0:
        assert abs(got_stat - ref["stat"]) <= rel_stat * ref["stat"] + 1e-300, (where, got_stat, ref["stat"], rel_stat)
        rel_p = (1.0 + ref["stat"] / 2.0) * rel_stat
        assert abs(got_p - ref["p"]) <= rel_p * ref["p"], (where, got_p, ref["p"], rel_p)
    assert abs(int(got_iters) - ref["iters"]) <= 1, (where, got_iters, ref["iters"])
    return eb, es


def check_row(rec, coef, e, where=""):
    """one hpgv_logistic_result record (and its coef (2, p) or None) against a row's expectation"""
    ref = e["fwd"]
    assert rec["n_obs"] == ref["n_obs"], (where, rec["n_obs"], ref["n_obs"])
    failed_nan = all(np.isnan(rec[k]) for k in ("beta", "se", "stat", "p")) and (coef is None or np.all(np.isnan(coef)))
    if e["kind"] == "ok":
        assert rec["status"] == OK, (where, rec["status"])
        check_numbers(rec["beta"], rec["se"], rec["stat"], rec["p"], rec["iters"], ref, where)
        if coef is not None:
            assert np.all(np.abs(coef[0] - ref["coef_beta"]) <= DEVICE_TOL * ref["coef_se"]), where
            assert np.all(np.abs(coef[1] - ref["coef_se"]) <= DEVICE_TOL * ref["coef_se"]), where
    elif e["kind"] == "singular":
        assert rec["status"] == SINGULAR and failed_nan, (where, rec["status"])
    elif e["kind"] == "nan":
        assert rec["status"] in (NOT_CONVERGED, SINGULAR) and failed_nan, (where, rec["status"])
    else:
        assert rec["status"] in (OK, NOT_CONVERGED, SINGULAR) and (rec["status"] == OK or failed_nan), (where, rec["status"])


def text_of(codes, chrom="7", pos0=100):
    """VCF data lines of a code matrix (alleles 0 .. 3, 15 = '.')"""
    names = {i: str(i) for i in range(15)}
    names[15] = "."
    return "".join("%s\t%d\trs%d\tA\tC,G,T\t.\tPASS\t.\tGT\t%s\n" % (chrom, pos0 + v, v, "\t".join(names[b >> 4] + "/" + names[b & 15] for b in row))
                   for v, row in enumerate(codes)).encode()


def format_f6(x):
    return "nan" if x != x else "%6f" % x


def format_line(chrom, pos, vid, ref, alt, r):
    """the runner's line for an oracle (or device) result r: a dict or record with n_obs, beta, se, stat, p, iters"""
    beta = float(r["beta"])
    orr = math.exp(beta) if beta == beta else math.nan
    return "\t".join([chrom, str(pos), vid, ref, alt, str(int(r["n_obs"])), format_f6(beta), format_f6(float(r["se"])), format_f6(orr),
                      format_f6(float(r["stat"])), format_f6(float(r["p"])), str(int(r["iters"]))])
