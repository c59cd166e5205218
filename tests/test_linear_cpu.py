"""The host pieces of the linear regression (include/hpgv.h "Linear regression"), which need no device: the exported symbols, the
conditions the oracle's cases must meet, the two yardsticks, hpgv_linear_fit against the extended-precision oracle on every case,
the statuses, the intercept's back-transform, hpgv_linear_t_p on the grid and against closed forms, and argument errors."""
import math
import os
import re

import numpy as np
import pytest

import linear_golden as ln
from helpers import hpgv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hpgv_set_phenotype", "hpgv_assoc_linear_dev", "hpgv_assoc_linear", "hpgv_assoc_linear_text", "hpgv_linear_fit", "hpgv_linear_t_p"]


@pytest.fixture(scope="module", autouse=True)
def built():
    hpgv.build()
    assert hasattr(hpgv.load(), "hpgv_linear_fit")         # (the oracle alone proves nothing about the library)


def test_the_symbols_are_exported_and_the_constants_are_the_headers():
    L = hpgv.load()
    for name in NEW:
        assert name in hpgv.SYMBOLS and hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "hpgv.h")).read()
    values = {k: int(v) for k, v in re.findall(r"HPGV_LINEAR_(\w+) = (\d+)", text)}
    assert values == dict(OK=hpgv.LINEAR_OK, SINGULAR=hpgv.LINEAR_SINGULAR, EXACT=hpgv.LINEAR_EXACT)
    assert (ln.OK, ln.SINGULAR, ln.EXACT) == (hpgv.LINEAR_OK, hpgv.LINEAR_SINGULAR, hpgv.LINEAR_EXACT) == (0, 1, 2)
    assert hpgv.LINEAR_RESULT.itemsize == 48 and hpgv.LINEAR_RESULT.fields["n_obs"][1] == 32 and hpgv.LINEAR_RESULT.fields["df"][1] == 36
    for name in ("linear_fit", "linear_t_p", "run_assoc_linear"):
        assert callable(getattr(hpgv, name))
    for name in ("set_phenotype", "assoc_linear", "assoc_linear_text", "assoc_linear_dev"):
        assert callable(getattr(hpgv.Engine, name))


def test_the_cases_meet_their_conditions():
    n_ok = n_well = 0
    for key in ln.CASES:
        case, exp = ln.expectations(*key)
        C = key[2]
        assert len(case["gt"]) == ln.N_ROWS + len(ln.named_rows(C)) and len(exp) == len(case["gt"]) - (C == 0)
        kinds = {e["name"]: e for e in exp[ln.N_ROWS:]}
        for name in ("all_missing", "monomorphic", "few_obs") + (("collinear_with_covariate",) if C else ()):
            assert kinds[name]["kind"] == "singular"
        coh = len(case["coh"])
        assert kinds["all_missing"]["ref"]["n_obs"] == 0 and kinds["no_missing"]["ref"]["n_obs"] == coh
        assert kinds["few_obs"]["ref"]["n_obs"] == min(C + 2, coh)
        mm = kinds["mostly_missing"]["ref"]["n_obs"]
        assert coh - mm > mm                              # the direct-sum branch
        if C:                                             # collinear in truth: the un-centred reference finds it singular too
            cls, y, cov = ln.cohort_view(case, kinds["collinear_with_covariate"]["row"])
            assert ln.ref_fit(cls, y, cov)["status"] == ln.SINGULAR and np.array_equal(cls[cls <= 2], cov[cls <= 2, 0] + 1)
        if ln.well_sized(*key):                           # a fit that fails everything cannot pass
            n_well += 1
            assert sum(e["kind"] == "ok" for e in exp[:ln.N_ROWS]) >= 0.9 * ln.N_ROWS, key
            assert kinds["byte_codes"]["kind"] == "ok" and kinds["no_missing"]["kind"] == "ok", key
            if mm >= 4 * (C + 2):
                assert kinds["mostly_missing"]["kind"] == "ok", key
        n_ok += sum(e["kind"] == "ok" for e in exp)
    assert n_well >= 17 and n_ok > 1400
    big = ln.make_case(300, 211, 3, "mean1000")
    yc = big["y"][big["coh"]]
    assert abs(yc.mean() - 1000.0) < 1e-9 and abs(yc.std() - 10.0) < 1e-9


def test_the_yardstick_covers_the_class_sums_in_both_directions():
    measured = ln.measure_E()
    print("E measured %.3g, constant %.3g, tolerance %.3g" % (measured, ln.E, ln.DEVICE_TOL))
    assert measured <= ln.E * 1.5 and measured >= ln.E / 8          # the constant is the measurement, give or take the BLAS at hand
    assert ln.DEVICE_TOL == max(64 * ln.E, 1e-12)


def test_the_tail_on_the_grid_and_its_yardstick():
    measured = ln.measure_tail(hpgv.linear_t_p)
    print("tail: worst relative deviation %.3g, constant %.3g, P tolerance %.3g" % (measured, ln.TAIL_DEV, ln.P_RTOL))
    assert measured <= ln.TAIL_DEV * 1.5 and ln.P_RTOL == max(1e-10, 4 * ln.TAIL_DEV)
    for df in ln.T_GRID_DF:
        for t in ln.T_GRID_T:
            ln.check_p(hpgv.linear_t_p(t, df), t, df, (t, df))
            assert hpgv.linear_t_p(-t, df) == hpgv.linear_t_p(t, df)


def test_the_tail_against_closed_forms_and_at_its_edges():
    for t in (0.0, 1e-8, 1e-3, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 40.0, 200.0, 1e6):
        one = 1.0 - 2.0 / math.pi * math.atan(t) if t < 1 else 2.0 / math.pi * math.atan(1.0 / t)
        two = 1.0 - t / math.sqrt(2.0 + t * t) if t < 1 else 2.0 / (math.sqrt(2.0 + t * t) * (t + math.sqrt(2.0 + t * t)))
        assert abs(hpgv.linear_t_p(t, 1) - one) <= 1e-12 * one, t
        assert abs(hpgv.linear_t_p(t, 2) - two) <= 1e-12 * two, t
    assert hpgv.linear_t_p(0.0, 7) == 1.0
    assert math.isnan(hpgv.linear_t_p(float("nan"), 5)) and math.isnan(hpgv.linear_t_p(1.0, 0)) and math.isnan(hpgv.linear_t_p(1.0, -3))
    assert hpgv.linear_t_p(float("inf"), 5) == 0.0 and hpgv.linear_t_p(-float("inf"), 5) == 0.0
    assert hpgv.linear_t_p(1e200, 3) == 0.0
    last = 1.0
    for t in np.linspace(0.01, 12, 200):                  # monotone through the switch between the two fractions
        now = hpgv.linear_t_p(t, 9)
        assert now < last
        last = now


@pytest.mark.parametrize("key", ln.CASES, ids=ln.case_id)
def test_the_host_fit_agrees_with_the_oracle(key):
    case, exp = ln.expectations(*key)
    worst, first_ok = 0.0, True
    for e in exp:
        cls, y, cov = ln.cohort_view(case, e["row"])
        rec, coef = hpgv.linear_fit(cls, y, cov)
        worst = max(worst, ln.check_row(rec, coef, e, (key, e["row"], e["name"])))
        if e["kind"] == "ok" and first_ok:                # and without coef the same record
            first_ok = False
            rec2 = np.zeros(1, hpgv.LINEAR_RESULT)
            cc, yy = np.ascontiguousarray(cov, np.float64), np.ascontiguousarray(y, np.float64)
            rc = hpgv.load().hpgv_linear_fit(hpgv._ptr(cls), hpgv._ptr(yy), hpgv._ptr(cc) if key[2] else None, len(cls), key[2], hpgv._ptr(rec2), None)
            assert rc == 0 and rec2[0].tobytes() == rec.tobytes()
    print("%s: worst deviation %.3g standard errors, tolerance %.3g" % (ln.case_id(key), worst, ln.DEVICE_TOL))
    if "exact_row" in case:
        cls, y, cov = ln.cohort_view(case, case["exact_row"], case["y_exact"])
        if (cls <= 2).sum() > 2 and len(set(cls[cls <= 2])) > 1:
            rec, coef = hpgv.linear_fit(cls, y, cov)
            ln.check_exact(rec, coef, key)


def test_the_statuses():
    case, exp = ln.expectations(129, 70, 3, "unit")
    got = {}
    for e in exp[ln.N_ROWS:]:
        cls, y, cov = ln.cohort_view(case, e["row"])
        got[e["name"]] = hpgv.linear_fit(cls, y, cov)
    for name in ("all_missing", "monomorphic", "collinear_with_covariate", "few_obs"):
        rec, coef = got[name]
        assert rec["status"] == ln.SINGULAR and np.isnan([rec["beta"], rec["se"], rec["stat"], rec["p"]]).all() and np.isnan(coef).all(), name
    assert got["all_missing"][0]["n_obs"] == 0 and got["all_missing"][0]["df"] == -5
    assert got["few_obs"][0]["n_obs"] == 5 and got["few_obs"][0]["df"] == 0
    assert got["monomorphic"][0]["n_obs"] > 150 and got["collinear_with_covariate"][0]["df"] > 150
    for name in ("mostly_missing", "no_missing", "byte_codes"):
        assert got[name][0]["status"] == ln.OK, name
    # df = 1 fits; a constant trait is an exact fit with beta 0
    cls = np.array([0, 1, 2, 255, 1], np.uint8)
    rec, coef = hpgv.linear_fit(cls, [1.0, 2.5, 3.0, 100.0, 2.0])
    ref = ln.ref_fit(cls, [1.0, 2.5, 3.0, 100.0, 2.0])
    assert rec["status"] == ln.OK and rec["df"] == 2 and abs(rec["beta"] - ref["beta"]) <= 1e-12 and abs(rec["se"] - ref["se"]) <= 1e-12
    rec, coef = hpgv.linear_fit(np.array([0, 1, 2], np.uint8), [1.0, 2.5, 3.0])
    assert rec["status"] == ln.OK and rec["df"] == 1
    rec, coef = hpgv.linear_fit(np.array([0, 1, 2, 1], np.uint8), [4.0, 4.0, 4.0, 4.0])
    assert rec["status"] == ln.EXACT and rec["beta"] == 0.0 and rec["se"] == 0.0 and np.isnan(rec["stat"]) and np.isnan(rec["p"])
    assert coef[0][0] == 4.0 and np.all(coef[1] == 0.0)


def test_the_intercept_is_that_of_the_uncentred_model():
    for key in [(300, 211, 3, "mean1000"), (129, 70, 14, "unit"), (64, 64, 0, "unit")]:
        case, exp = ln.expectations(*key)
        for e in exp[:ln.N_ROWS:9]:
            if e["kind"] != "ok":
                continue
            cls, y, cov = ln.cohort_view(case, e["row"])
            rec, coef = hpgv.linear_fit(cls, y, cov)
            obs = cls <= 2
            X = np.column_stack([np.ones(obs.sum()), cls[obs].astype(float), cov[obs]])
            beta, res = np.linalg.lstsq(X, y[obs], rcond=None)[:2]        # numpy's own solver, un-centred
            V = np.linalg.inv(X.T @ X) * res[0] / (obs.sum() - X.shape[1])
            assert np.allclose(coef[0], beta, rtol=0, atol=1e-8 * np.sqrt(np.diag(V)).max())
            assert np.allclose(coef[1], np.sqrt(np.diag(V)), rtol=1e-8)
            if key[3] == "mean1000":
                assert abs(coef[0][0] - 1000.0) < 20.0
            # a shift of the trait moves the intercept alone, a shift of a covariate too
            rec2, coef2 = hpgv.linear_fit(cls, y + 250.0, cov)
            assert abs(coef2[0][0] - coef[0][0] - 250.0) <= 1e-9 and np.allclose(coef2[0][1:], coef[0][1:], rtol=0, atol=1e-10)
            assert np.allclose(coef2[1], coef[1], rtol=1e-9)


def test_argument_errors():
    L = hpgv.load()
    cls, y = np.zeros(4, np.uint8), np.zeros(4)
    cov = np.zeros((4, 15))
    out = np.zeros(1, hpgv.LINEAR_RESULT)
    p = hpgv._ptr
    bad = [(p(cls), p(y), None, -1, 0, p(out)), (p(cls), p(y), p(cov), 4, 15, p(out)), (p(cls), p(y), None, 4, -1, p(out)), (p(cls), p(y), None, 4, 0, None),
           (None, p(y), None, 4, 0, p(out)), (p(cls), None, None, 4, 0, p(out)), (p(cls), p(y), None, 4, 2, p(out))]
    for args in bad:
        assert L.hpgv_linear_fit(*args, None) == hpgv.ERR_INVALID, args[3:5]
    for word in (np.nan, np.inf, -np.inf):
        y2 = y.copy()
        y2[2] = word
        assert L.hpgv_linear_fit(p(cls), p(y2), None, 4, 0, p(out), None) == hpgv.ERR_INVALID
        c2 = np.zeros((4, 2))
        c2[1, 1] = word
        assert L.hpgv_linear_fit(p(cls), p(y), p(c2), 4, 2, p(out), None) == hpgv.ERR_INVALID
    assert L.hpgv_linear_fit(None, None, None, 0, 0, p(out), None) == 0 and out[0]["status"] == ln.SINGULAR and out[0]["n_obs"] == 0 and out[0]["df"] == -2
