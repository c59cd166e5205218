"""The host pieces of the logistic regression (include/hpgv.h "Logistic regression"), which need no device: the exported symbols,
the conditions the oracle's cases must meet (every shipped kernel shape among them), hpgv_logistic_fit against the oracle, against
the score equation and against a scipy.optimize fit of the same likelihood, the status rows, argument errors, and the
covariate-file reader."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import logistic_golden as lg
from helpers import hpgv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hpgv_set_covariates", "hpgv_assoc_logistic_dev", "hpgv_assoc_logistic", "hpgv_assoc_logistic_text", "hpgv_logistic_fit"]


@pytest.fixture(scope="module", autouse=True)
def built():
    hpgv.build()
    assert hasattr(hpgv.load(), "hpgv_logistic_fit")       # (the oracle alone proves nothing about the library)


def test_the_symbols_are_exported_and_the_constants_are_the_headers():
    L = hpgv.load()
    for name in NEW:
        assert name in hpgv.SYMBOLS and hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "hpgv.h")).read()
    assert int(re.search(r"HPGV_LOGISTIC_MAX_COVAR = (\d+)", text).group(1)) == hpgv.LOGISTIC_MAX_COVAR == lg.MAX_COVAR == 14
    values = {k: int(v) for k, v in re.findall(r"HPGV_LOGIT_(\w+) = (\d+)", text)}
    assert values == dict(OK=hpgv.LOGIT_OK, NOT_CONVERGED=hpgv.LOGIT_NOT_CONVERGED, SINGULAR=hpgv.LOGIT_SINGULAR)
    assert (lg.OK, lg.NOT_CONVERGED, lg.SINGULAR) == (0, 1, 2)
    assert hpgv.LOGISTIC_RESULT.itemsize == 48 and hpgv.LOGISTIC_RESULT.fields["n_obs"][1] == 32
    host = open(os.path.join(ROOT, "include", "hpgv_host.h")).read()
    assert int(re.search(r"HPGV_RUN_LOGISTIC_MAX_ITER (\d+)", host).group(1)) == lg.MAX_ITER
    assert float(re.search(r"HPGV_RUN_LOGISTIC_TOL (\S+)", host).group(1)) == lg.TOL
    for name in ("logistic_fit", "run_assoc_logistic", "covar_read"):
        assert callable(getattr(hpgv, name))
    for name in ("set_covariates", "assoc_logistic", "assoc_logistic_text", "assoc_logistic_dev"):
        assert callable(getattr(hpgv.Engine, name))


def test_the_cases_meet_their_conditions():
    n_ok = 0
    for key in lg.CASES:
        case, exp = lg.expectations(*key)
        assert len(exp) == lg.N_ROWS + len(lg.STATUS_ROWS)
        for r, e in enumerate(exp):
            f, b = e["fwd"], e["rev"]
            assert f["n_obs"] == b["n_obs"]
            if e["kind"] == "ok":
                assert f["status"] == b["status"] == lg.OK and min(f["ratio"], b["ratio"]) > 1e-6 and max(f["iters"], b["iters"]) <= 12
                n_ok += 1
            elif e["kind"] == "singular":         # singular by construction, and the oracle finds it so in both orders
                assert f["status"] == b["status"] == lg.SINGULAR, (key, r, e["name"])
            elif e["kind"] == "nan":
                assert f["status"] != lg.OK and b["status"] != lg.OK
        names = {e["name"]: e["kind"] for e in exp[lg.N_ROWS:]}
        assert names["all_missing"] == names["monomorphic"] == names["monomorphic_alt"] == names["few_obs"] == "singular"
        assert names["separated"] in ("nan", "singular") and names["one_class"] in ("nan", "singular") and names["single_het"] in ("nan", "singular")
        if lg.well_sized(*key):                   # a fit that fails everything cannot pass
            random_ok = sum(e["kind"] == "ok" for e in exp[:lg.N_ROWS])
            assert random_ok >= 0.9 * lg.N_ROWS, (key, random_ok)
            assert names["byte_codes"] == "ok", key
    assert sum(lg.well_sized(*k) for k in lg.CASES) >= 15 and n_ok > 1500


def test_every_shipped_kernel_shape_has_well_sized_cases_and_the_nested_ones_meet_their_conditions():
    """by p = C + 2 as logistic_launch dispatches: every instantiation, every P filled exactly, pads of 1 and of 3 coordinates --
    each with well-sized cases, whose random rows the oracle alone fits nine times in ten"""
    shipped = [2, 4, 6, 8, 12, 16]
    well = {}
    for nA, nU, C in lg.CASES:
        if lg.well_sized(nA, nU, C):
            P = min(P for P in shipped if P >= C + 2)
            well.setdefault((P, P - C - 2), []).append((nA, nU))
    for P in shipped:
        assert len(well.get((P, 0), [])) >= 2, P                   # p fills P
    for P in shipped[1:]:
        assert len(well.get((P, 1), [])) >= 2, P                   # one pad coordinate
    assert len(well[(12, 3)]) >= 2
    for C in lg.COVARS_LONG:                                       # the long cohort: one case per DEAL, and <8,1>
        assert lg.well_sized(*lg.LONG, C) and lg.LONG + (C,) in lg.CASES
    assert lg.well_sized(*lg.NESTED) and lg.COVARS_NESTED == [6, 7, 10, 11]
    wide, _ = lg.nested_expectations(lg.NESTED[2])
    for C in lg.COVARS_NESTED:
        case, exp = lg.nested_expectations(C)
        assert case["cov"].shape[1] == C and len(exp) == len(case["gt"]) == lg.N_ROWS
        assert np.array_equal(case["cov"], wide["cov"][:, :C], equal_nan=True) and np.array_equal(case["gt"], wide["gt"])
        assert sum(e["kind"] == "ok" for e in exp) >= 0.9 * lg.N_ROWS, C
        for r in range(0, lg.N_ROWS, 4):                           # and the host fit, which shares logit_chol_inv with the kernel
            cls, y, cov = lg.cohort_view(case, r)
            rec, coef = hpgv.logistic_fit(cls, y, cov)
            lg.check_row(rec, coef, exp[r], (C, r))


def test_the_yardstick_covers_the_two_summation_orders():
    measured = lg.measure_E()
    print("E measured %.3g, constant %.3g, device tolerance %.3g" % (measured, lg.E, lg.DEVICE_TOL))
    assert measured <= lg.E * 1.5 and measured >= lg.E / 8        # the constant is the measurement, give or take the BLAS at hand
    assert lg.DEVICE_TOL == max(64 * lg.E, 1e-12)


@pytest.mark.parametrize("key", lg.CASES, ids=lambda k: "%dx%d_C%d" % k)
def test_the_host_fit_agrees_with_the_oracle(key):
    case, exp = lg.expectations(*key)
    first_ok = True
    for r, e in enumerate(exp):
        cls, y, cov = lg.cohort_view(case, r)
        rec, coef = hpgv.logistic_fit(cls, y, cov)
        lg.check_row(rec, coef, e, (key, r, e["name"]))
        if e["kind"] == "ok" and first_ok:        # and without coef the same record
            first_ok = False
            rec2 = np.zeros(1, hpgv.LOGISTIC_RESULT)
            cc = np.ascontiguousarray(cov, np.float64)
            rc = hpgv.load().hpgv_logistic_fit(hpgv._ptr(cls), hpgv._ptr(y), hpgv._ptr(cc) if key[2] else None, len(cls), key[2], lg.MAX_ITER, lg.TOL,
                                               hpgv._ptr(rec2), None)
            assert rc == 0 and rec2[0].tobytes() == rec.tobytes()


def test_the_score_vanishes_at_the_fit():
    """u(beta) recomputed in numpy from the returned coefficients: not the oracle's solver"""
    for key in [(37, 29, 3), (129, 70, 14), (300, 211, 0), (300, 211, 13), (129, 70, 6), (300, 211, 9), (129, 70, 10), (700, 600, 10)]:
        case, exp = lg.expectations(*key)
        for r in range(0, lg.N_ROWS, 7):
            if exp[r]["kind"] != "ok":
                continue
            cls, y, cov = lg.cohort_view(case, r)
            rec, coef = hpgv.logistic_fit(cls, y, cov)
            obs = cls <= 2
            X = np.column_stack([np.ones(obs.sum()), cls[obs].astype(float), cov[obs]])
            mu = 1.0 / (1.0 + np.exp(-(X @ coef[0])))
            u = X.T @ (y[obs] - mu)
            assert np.max(np.abs(u)) < 1e-8 * obs.sum(), (key, r, u)
            H = (X * (mu * (1 - mu))[:, None]).T @ X
            assert np.allclose(np.sqrt(np.diag(np.linalg.inv(H))), coef[1], rtol=1e-7)


def test_a_scipy_fit_of_the_same_likelihood_agrees():
    from scipy.optimize import minimize
    for key, r in [((300, 211, 3), 0), ((129, 70, 1), 5), ((64, 64, 0), 11), ((300, 211, 6), 2), ((300, 211, 10), 4), ((700, 600, 6), 9)]:
        case, exp = lg.expectations(*key)
        assert exp[r]["kind"] == "ok"
        cls, y, cov = lg.cohort_view(case, r)
        obs = cls <= 2
        X = np.column_stack([np.ones(obs.sum()), cls[obs].astype(float), cov[obs]])
        yy = y[obs].astype(float)

        def nll(b):
            eta = X @ b
            return np.sum(np.logaddexp(0.0, eta) - yy * eta)

        def grad(b):
            return X.T @ (1.0 / (1.0 + np.exp(-(X @ b))) - yy)

        best = minimize(nll, np.zeros(X.shape[1]), jac=grad, method="BFGS", options=dict(gtol=1e-10, maxiter=2000))
        best = minimize(nll, best.x, jac=grad, method="Newton-CG", tol=1e-14, options=dict(xtol=1e-14, maxiter=200))
        rec, coef = hpgv.logistic_fit(cls, y, cov)
        assert np.max(np.abs(best.x - coef[0])) < 1e-6, (key, r, best.x, coef[0])


def test_the_status_rows():
    case, exp = lg.expectations(129, 70, 3)
    got = {}
    for r in range(lg.N_ROWS, len(exp)):
        cls, y, cov = lg.cohort_view(case, r)
        rec, coef = hpgv.logistic_fit(cls, y, cov)
        got[exp[r]["name"]] = rec
        if exp[r]["kind"] != "ok":
            assert np.isnan([rec["beta"], rec["se"], rec["stat"], rec["p"]]).all() and np.isnan(coef).all()
    assert got["all_missing"]["status"] == lg.SINGULAR and got["all_missing"]["n_obs"] == 0 and got["all_missing"]["iters"] == 0
    assert got["monomorphic"]["status"] == got["monomorphic_alt"]["status"] == got["few_obs"]["status"] == lg.SINGULAR
    assert got["few_obs"]["n_obs"] == 4
    assert got["separated"]["status"] in (lg.NOT_CONVERGED, lg.SINGULAR) and got["one_class"]["status"] in (lg.NOT_CONVERGED, lg.SINGULAR)
    assert got["single_het"]["status"] in (lg.NOT_CONVERGED, lg.SINGULAR)
    assert got["byte_codes"]["status"] == lg.OK and got["byte_codes"]["n_obs"] == int((lg.classify(case["gt"][-1, case["coh"]]) <= 2).sum())
    # max_iter steps without convergence: NOT_CONVERGED with iters = max_iter; one step more than the fit needs: OK
    cls, y, cov = lg.cohort_view(case, 0)
    full, _ = hpgv.logistic_fit(cls, y, cov)
    assert full["status"] == lg.OK and full["iters"] >= 3
    short, _ = hpgv.logistic_fit(cls, y, cov, max_iter=int(full["iters"]) - 1)
    assert short["status"] == lg.NOT_CONVERGED and short["iters"] == full["iters"] - 1 and np.isnan(short["beta"])
    exact, _ = hpgv.logistic_fit(cls, y, cov, max_iter=int(full["iters"]))
    assert exact.tobytes() == full.tobytes()


def test_argument_errors():
    L = hpgv.load()
    cls, y = np.zeros(4, np.uint8), np.zeros(4, np.uint8)
    cov = np.zeros((4, 15))
    out = np.zeros(1, hpgv.LOGISTIC_RESULT)
    p = hpgv._ptr
    bad = [(p(cls), p(y), None, -1, 0, 25, 1e-10, p(out)), (p(cls), p(y), p(cov), 4, 15, 25, 1e-10, p(out)), (p(cls), p(y), None, 4, -1, 25, 1e-10, p(out)),
           (p(cls), p(y), None, 4, 0, 0, 1e-10, p(out)), (p(cls), p(y), None, 4, 0, 101, 1e-10, p(out)), (p(cls), p(y), None, 4, 0, 25, -1.0, p(out)),
           (p(cls), p(y), None, 4, 0, 25, float("nan"), p(out)), (p(cls), p(y), None, 4, 0, 25, float("inf"), p(out)), (p(cls), p(y), None, 4, 0, 25, 1e-10, None),
           (None, p(y), None, 4, 0, 25, 1e-10, p(out)), (p(cls), None, None, 4, 0, 25, 1e-10, p(out)), (p(cls), p(y), None, 4, 2, 25, 1e-10, p(out))]
    for args in bad:
        assert L.hpgv_logistic_fit(*args, None) == hpgv.ERR_INVALID, args[3:7]
    assert L.hpgv_logistic_fit(None, None, None, 0, 0, 25, 1e-10, p(out), None) == 0 and out[0]["status"] == lg.SINGULAR and out[0]["n_obs"] == 0
    assert L.hpgv_logistic_fit(p(cls), p(y), None, 4, 0, 100, 0.0, p(out), None) == 0


# ---- the covariate file ------------------------------------------------------------------------------------------------------

NAMES = ["s1", "s2", "s3", "s4"]


def _covar(tmp_path, text, n_covar=0, names=NAMES):
    path = tmp_path / "covar.txt"
    path.write_text(text)
    return hpgv.covar_read(str(path), names, n_covar)


@pytest.mark.parametrize("header", ["", "FID IID PC1 PC2\n", "#FID\tIID\tPC1\tPC2\n", "#IID IID2 A B\n"])
def test_covariate_file_header_forms(tmp_path, header):
    cov, have = _covar(tmp_path, header + "f s2 1.5 -2\nf s1\t0.25   4e-1\n\nf zz 9 9\nf s4 1 NA\n")
    assert cov.shape == (4, 2) and list(have) == [1, 1, 0, 0]
    assert np.array_equal(cov, [[0.25, 0.4], [1.5, -2.0], [0, 0], [0, 0]])
    cov1, have1 = _covar(tmp_path, header + "f s2 1.5 -2\nf s1\t0.25   4e-1\nf s4 1 NA\n", n_covar=1)
    assert cov1.shape == (4, 1) and list(have1) == [1, 1, 0, 1] and cov1[3, 0] == 1.0      # the NA is in a column not in use


def test_covariate_file_eigenvec_shape_and_values_that_are_no_numbers(tmp_path):
    text = "".join("%s\t%s\t%.8g\t%.8g\t%.8g\n" % (n, n, 0.1 * i, -0.01 * i, 1e-3) for i, n in enumerate(NAMES))
    cov, have = _covar(tmp_path, text)
    assert have.all() and np.allclose(cov[:, 0], [0, 0.1, 0.2, 0.3]) and cov.shape == (4, 3)
    for word in ("NA", "nan", "inf", "-inf", "1.5x", "."):
        cov, have = _covar(tmp_path, "a s1 1 2\na s2 %s 2\na s3 3 4\n" % word)
        assert list(have) == [1, 0, 1, 0], word
    cov, have = _covar(tmp_path, "FID IID\na s1\na s2\n")               # ids only: no columns, every listed sample has a line
    assert cov.shape == (4, 0) and list(have) == [1, 1, 0, 0]


@pytest.mark.parametrize("text,n_covar", [("a s1 1 2\nb s1 3 4\n", 0),                                      # a duplicate id
                                          ("a s1 1 2\na s2 3\n", 0), ("a s1 1\na s2 3 4\n", 0),              # ragged
                                          ("a s1 1 2\na\n", 0),                                              # no second id
                                          ("a s1 " + " ".join(["1"] * 15) + "\n", 0),                        # 15 columns in use
                                          ("a s1 1 2\n", 3), ("a s1 1 2\n", 15), ("a s1 1 2\n", -1)])
def test_covariate_file_errors(tmp_path, text, n_covar):
    with pytest.raises(hpgv.HpgvError) as err:
        _covar(tmp_path, text, n_covar)
    assert err.value.code == hpgv.ERR_INVALID


def test_covariate_file_limits_and_missing_file(tmp_path):
    cov, have = _covar(tmp_path, "a s1 " + " ".join(str(k) for k in range(15)) + "\n", n_covar=14)      # 15 columns, 14 in use
    assert cov.shape == (4, 14) and np.array_equal(cov[0], np.arange(14.0)) and list(have) == [1, 0, 0, 0]
    with pytest.raises(hpgv.HpgvError) as err:
        hpgv.covar_read(str(tmp_path / "none.txt"), NAMES)
    assert err.value.code == hpgv.ERR_INVALID
    with pytest.raises(hpgv.HpgvError):
        hpgv.covar_read(None, NAMES)
