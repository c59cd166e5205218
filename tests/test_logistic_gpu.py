"""The logistic regression on the device (include/hpgv.h "Logistic regression"): k_logistic through hpgv_assoc_logistic_dev, the
host-batch and the text entry points against the numpy oracle of logistic_golden under its tolerances -- every cohort shape that
moves the pads, the lane steps and the ragged last step, every instantiation of k_logistic<P, DEAL> with p filling P and with pad
coordinates, one cohort long enough for several turns of every wave's sample loop -- then the dispatch edges on nested covariate
columns, bit identity of split calls and repeated runs, a stream of the caller's, the covariates' life with the cohort, and the error codes."""
import ctypes as C

import numpy as np
import pytest

import logistic_golden as lg
from helpers import hpgv

pytestmark = pytest.mark.gpu

N_ALL = lg.N_ROWS + len(lg.STATUS_ROWS)


def engine(case, covariates=True):
    e = hpgv.Engine(0)
    nA, nU, _ = e.set_cohort(case["cond"])
    assert (nA, nU) == (case["nA"], case["nU"])
    if covariates and case["C"]:
        e.set_covariates(case["cov"])                     # NaN in the OTHER columns: ignored
    return e


def run_dev(e, case, rows=slice(None), coef=True, stream=None, C_=None):
    """layout and k_logistic on device buffers: (records, coef (nv, 2, p) or None)"""
    codes = np.ascontiguousarray(case["gt"][rows])
    nv, ns, p = len(codes), codes.shape[1], (case["C"] if C_ is None else C_) + 2
    pitch = e.assoc_layout()[2]
    bufs = [e.alloc(max(n, 16)) for n in (nv * ns, nv * pitch, nv * 48, nv * 2 * p * 8)]
    d_raw, d_lay, d_out, d_coef = bufs
    e.h2d(d_raw, codes)
    e.layout(hpgv.LAYOUT_ASSOC, d_raw, ns, nv, d_lay)
    e.sync()
    e.h2d(d_out, np.full(nv * 48, 0xAB, np.uint8))
    e.assoc_logistic_dev(d_lay, nv, d_out, d_coef if coef else None, lg.MAX_ITER, lg.TOL, stream=stream)
    e.sync(stream)
    out = e.d2h(d_out, (nv,), hpgv.LOGISTIC_RESULT)
    cf = e.d2h(d_coef, (nv, 2, p), np.float64) if coef else None
    for b in bufs:
        e.free(b)
    return out, cf


def same(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("key", lg.CASES, ids=lambda k: "%dx%d_C%d" % k)
def test_the_three_entry_points_against_the_oracle(key):
    case, exp = lg.expectations(*key)
    e = engine(case)
    out, cf = run_dev(e, case)
    worst_b = worst_s = 0.0
    for r, x in enumerate(exp):
        lg.check_row(out[r], cf[r], x, (key, r, x["name"]))
        assert out[r]["pad"] == 0
        if x["kind"] == "ok":
            worst_b = max(worst_b, np.max(np.abs(cf[r][0] - x["fwd"]["coef_beta"]) / x["fwd"]["coef_se"]))
            worst_s = max(worst_s, np.max(np.abs(cf[r][1] - x["fwd"]["coef_se"]) / x["fwd"]["coef_se"]))
            assert cf[r][0][1] == out[r]["beta"] and cf[r][1][1] == out[r]["se"]
    print("%s: worst |d beta| / se %.3g, |d se| / se %.3g, tolerance %.3g" % (key, worst_b, worst_s, lg.DEVICE_TOL))
    if lg.well_sized(*key):
        assert (out["status"][:lg.N_ROWS] == lg.OK).sum() >= 0.9 * lg.N_ROWS
    # d_coef NULL: the same records; the host batch and the text: the same records and coefficients, bit for bit
    plain, none = run_dev(e, case, coef=False)
    assert same(plain, out) and none is None
    hb, hc = e.assoc_logistic(case["gt"], coef=True)
    assert same(hb, out) and same(hc, cf)
    assert same(e.assoc_logistic(case["gt"]), out)
    rt = e.assoc_logistic_text(lg.text_of(case["gt"]), coef=True)
    assert rt["n_lines"] == N_ALL and not rt["status"].any()
    assert same(rt["out"], out) and same(rt["coef"], cf)
    e.close()


def test_the_long_cohort_takes_every_kernel_through_several_ragged_turns():
    """what the LONG cases of test_the_three_entry_points_against_the_oracle rest on: a pitch above 1024 positions, so that the
    sample loop of logit_pass -- 64 * NSUB pairs per turn -- takes 3 turns in its first waves and lanes and 2 in the others with
    DEAL = 1, 5 or 6 with DEAL = 2, 10 or 11 with DEAL = 4"""
    case, _ = lg.expectations(*lg.LONG, lg.COVARS_LONG[0])
    e = engine(case, covariates=False)
    pitch = e.assoc_layout()[2]
    e.close()
    assert pitch > 1024 and pitch % 16 == 0
    for deal, turns in ((1, (2, 3)), (2, (5, 6)), (4, (10, 11))):
        step = 64 * (4 // deal)                            # pairs of positions per turn
        assert (pitch // 2) % step != 0                    # ragged
        assert ((pitch // 2) // step, -(-(pitch // 2) // step)) == turns, (deal, pitch)
    assert [C_ for C_ in lg.COVARS_LONG if lg.LONG + (C_,) in lg.CASES] == [3, 6, 10, 14]       # <6,1>, <8,1>, <12,2>, <16,4>


@pytest.mark.parametrize("key", [(37, 29, 3), (129, 70, 13), (300, 211, 14), (15, 17, 0), (129, 70, 6), (300, 211, 10)],
                         ids=lambda k: "%dx%d_C%d" % k)
def test_split_calls_and_repeated_runs_are_bit_identical(key):
    case, _ = lg.expectations(*key)
    e = engine(case)
    whole, wc = run_dev(e, case)
    again, ac = run_dev(e, case)
    assert same(whole, again) and same(wc, ac)
    for pieces in ((1, 5, 67), (1, 5, 15, 16, 17)):        # n_variants 1, 5 and 67, or 1, 5, 15, 16 and 17, then the rest
        at = 0
        for nv in pieces + (N_ALL - sum(pieces),):
            part, pc = run_dev(e, case, slice(at, at + nv))
            assert same(part, whole[at:at + nv]) and same(pc, wc[at:at + nv]), (at, nv)
            at += nv
        assert at == N_ALL
    e.close()


def test_the_dispatch_edges_on_nested_covariates():
    """One cohort, the same rows, the first 6, 7, 10 and 11 columns of one covariate matrix: k_logistic<8,1> | <12,2> | <16,4>.
    Every fit agrees with its own oracle fit, so an error of one instantiation is a jump at its edge: the figures are printed side
    by side."""
    e, ref = None, None
    for C_ in lg.COVARS_NESTED:
        case, exp = lg.nested_expectations(C_)
        if e is None:
            e = engine(case, covariates=False)
        e.set_covariates(case["cov"])
        out, cf = run_dev(e, case)
        assert cf.shape == (lg.N_ROWS, 2, C_ + 2)
        worst_b = worst_s = 0.0
        n_ok = 0
        for r, x in enumerate(exp):
            lg.check_row(out[r], cf[r], x, (C_, r))
            if x["kind"] == "ok":
                n_ok += 1
                worst_b = max(worst_b, np.max(np.abs(cf[r][0] - x["fwd"]["coef_beta"]) / x["fwd"]["coef_se"]))
                worst_s = max(worst_s, np.max(np.abs(cf[r][1] - x["fwd"]["coef_se"]) / x["fwd"]["coef_se"]))
        print("C = %d: %d rows ok, worst |d beta| / se %.3g, |d se| / se %.3g, tolerance %.3g" % (C_, n_ok, worst_b, worst_s, lg.DEVICE_TOL))
        assert n_ok >= 0.9 * lg.N_ROWS and (out["status"] == lg.OK).sum() >= 0.9 * lg.N_ROWS
        if ref is not None:                                # the same genotypes: the same observations at every C
            assert np.array_equal(out["n_obs"], ref["n_obs"]) and not same(out["beta"], ref["beta"])
        ref = out
    e.close()


def test_a_stream_of_the_callers():
    case, exp = lg.expectations(64, 64, 3)
    e = engine(case)
    ref, rc = run_dev(e, case)
    s = C.c_void_p()
    assert e.L.hpgv_stream_create(e.h, C.byref(s)) == hpgv.OK
    got, gc = run_dev(e, case, stream=s)
    assert e.L.hpgv_stream_destroy(e.h, s) == hpgv.OK
    assert same(got, ref) and same(gc, rc)
    e.close()


def test_covariates_of_other_columns_are_ignored_and_a_new_cohort_drops_them():
    case, exp = lg.expectations(37, 29, 3)
    e = engine(case)
    ref, _ = run_dev(e, case)
    cov = case["cov"].copy()
    cov[case["cond"] == 2] = 123.0                         # any value: the same records
    e.set_covariates(cov)
    assert same(run_dev(e, case)[0], ref)
    # without covariates: C = 0, the records of the (37, 29, 0) fit on the same rows
    e.set_covariates(None)
    base, bc = run_dev(e, case, C_=0)
    assert bc.shape == (N_ALL, 2, 2) and not same(base, ref)
    for r in range(lg.N_ROWS):
        cls, y, _ = lg.cohort_view(case, r)
        o = lg.fit(cls, y)
        assert o["status"] == lg.OK and base[r]["status"] == lg.OK
        lg.check_numbers(base[r]["beta"], base[r]["se"], base[r]["stat"], base[r]["p"], base[r]["iters"], o, r)
    e.set_covariates(case["cov"])
    assert same(run_dev(e, case)[0], ref)
    e.set_cohort(case["cond"])                             # the same cohort set again: the covariates are gone all the same
    assert same(run_dev(e, case, C_=0)[0], base)
    assert same(e.assoc_logistic(case["gt"]), base)
    e.close()


def test_a_group_context_gives_every_member_the_covariates():
    case, _ = lg.expectations(37, 29, 3)
    e = engine(case)
    ref, rc = e.assoc_logistic(case["gt"], coef=True)
    e.close()
    g = hpgv.Engine([0, 0])
    g.set_cohort(case["cond"])
    g.set_covariates(case["cov"])
    text = lg.text_of(case["gt"])
    for _ in range(3):                                     # dealt to either member
        out, cf = g.assoc_logistic(case["gt"], coef=True)
        assert same(out, ref) and same(cf, rc)
        assert same(g.assoc_logistic_text(text)["out"], ref)
    assert same(run_dev(g.member(1), case)[0], ref)       # the second member's own state, through its *_dev call
    g.close()


def test_error_codes():
    case, _ = lg.expectations(15, 17, 1)
    L = hpgv.load()
    e = hpgv.Engine(0)
    n = len(case["cond"])
    cov = np.ascontiguousarray(np.nan_to_num(case["cov"]))
    p = hpgv._ptr
    out = np.zeros(4, hpgv.LOGISTIC_RESULT)
    gt = np.ascontiguousarray(case["gt"][:4])
    nl = C.c_int(0)
    # before a cohort
    assert L.hpgv_set_covariates(e.h, p(cov), n, 1) == hpgv.ERR_STATE
    assert L.hpgv_assoc_logistic(e.h, p(gt), n, 4, 25, 1e-10, p(out), None) == hpgv.ERR_STATE
    assert L.hpgv_assoc_logistic_dev(e.h, None, 0, 25, 1e-10, None, None, None) == hpgv.ERR_STATE
    assert L.hpgv_assoc_logistic_text(e.h, b"", 0, 0, C.byref(nl), None, None, None, 25, 1e-10, None, None) == hpgv.ERR_STATE
    e.set_cohort(case["cond"])
    assert L.hpgv_set_covariates(e.h, p(cov), n - 1, 1) == hpgv.ERR_INVALID
    assert L.hpgv_set_covariates(e.h, p(cov), n + 1, 1) == hpgv.ERR_INVALID
    assert L.hpgv_set_covariates(e.h, None, n, 1) == hpgv.ERR_INVALID
    assert L.hpgv_set_covariates(e.h, p(cov), n, -1) == hpgv.ERR_INVALID
    wide = np.zeros((n, 15))
    assert L.hpgv_set_covariates(e.h, p(wide), n, 15) == hpgv.ERR_UNSUPPORTED
    assert L.hpgv_set_covariates(e.h, p(np.zeros((n, 14))), n, 14) == hpgv.OK
    for bad in (np.nan, np.inf, -np.inf):
        c2 = cov.copy()
        c2[case["coh"][3], 0] = bad                        # a cohort column
        assert L.hpgv_set_covariates(e.h, p(c2), n, 1) == hpgv.ERR_INVALID
        assert b"not finite" in L.hpgv_last_error(e.h)
    c2 = cov.copy()
    c2[case["cond"] == 2] = np.inf                         # OTHER columns may hold anything
    assert L.hpgv_set_covariates(e.h, p(c2), n, 1) == hpgv.OK
    assert L.hpgv_set_covariates(e.h, None, 0, 0) == hpgv.OK      # clears, whatever n_samples says
    d = e.alloc(4096)
    for max_iter, tol in ((0, 1e-10), (101, 1e-10), (-3, 1e-10), (25, -1e-10), (25, float("nan")), (25, float("inf"))):
        assert L.hpgv_assoc_logistic_dev(e.h, d, 1, max_iter, tol, d, None, None) == hpgv.ERR_INVALID
        assert L.hpgv_assoc_logistic(e.h, p(gt), n, 4, max_iter, tol, p(out), None) == hpgv.ERR_INVALID
        assert L.hpgv_assoc_logistic_text(e.h, b"x\n", 2, 1, C.byref(nl), None, None, None, max_iter, tol, p(out), None) == hpgv.ERR_INVALID
    odd = C.c_void_p(d.value + 8)
    assert L.hpgv_assoc_logistic_dev(e.h, odd, 1, 25, 1e-10, d, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_logistic_dev(e.h, d, 1, 25, 1e-10, odd, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_logistic_dev(e.h, d, 1, 25, 1e-10, d, C.c_void_p(d.value + 4), None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_logistic_dev(e.h, d, -1, 25, 1e-10, d, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_logistic_dev(e.h, None, 1, 25, 1e-10, d, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_logistic_dev(e.h, d, 1, 25, 1e-10, None, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_logistic_dev(e.h, None, 0, 25, 1e-10, None, None, None) == hpgv.OK
    assert L.hpgv_assoc_logistic(e.h, p(gt), n - 1, 4, 25, 1e-10, p(out), None) == hpgv.ERR_INVALID      # pitch below n_samples
    assert L.hpgv_assoc_logistic(e.h, None, n, 4, 25, 1e-10, p(out), None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_logistic(e.h, p(gt), n, 4, 25, 1e-10, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_logistic(e.h, None, n, 0, 25, 1e-10, None, None) == hpgv.OK
    assert L.hpgv_assoc_logistic_text(e.h, b"x\n", 2, 1, None, None, None, None, 25, 1e-10, p(out), None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_logistic_text(e.h, b"x\n", 2, 1, C.byref(nl), None, None, None, 25, 1e-10, None, None) == hpgv.ERR_INVALID
    e.close()
