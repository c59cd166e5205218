"""The linear regression on the device (include/hpgv.h "Linear regression"): k_linear through hpgv_assoc_linear_dev, the host-batch
and the text entry points against the extended-precision oracle of linear_golden under its tolerances -- every cohort shape that
moves the segment pad, the 16-byte load, the 64-position wave step and the ragged last k-step, with 0 to 14 covariates -- then bit
identity of split calls and repeated runs, a stream of the caller's, the image following the set calls in either order, the
phenotype's life with the cohort, and the error codes."""
import ctypes as C

import numpy as np
import pytest

import linear_golden as ln
from helpers import hpgv

pytestmark = pytest.mark.gpu


def engine(case, y=None, order="cohort,covariates,phenotype"):
    e = hpgv.Engine(0)
    for step in order.split(","):
        if step == "cohort":
            nA, nU, _ = e.set_cohort(case["cond"])
            assert (nA, nU) == (case["nA"], case["nU"])
        elif step == "covariates" and case["C"]:
            e.set_covariates(case["cov"])                 # NaN in the OTHER columns: ignored
        elif step == "phenotype":
            e.set_phenotype(case["y"] if y is None else y)
    return e


def run_dev(e, case, rows=slice(None), coef=True, stream=None, C_=None):
    """layout and k_linear on device buffers: (records, coef (nv, 2, p) or None)"""
    codes = np.ascontiguousarray(case["gt"][rows])
    nv, ns, p = len(codes), codes.shape[1], (case["C"] if C_ is None else C_) + 2
    pitch = e.assoc_layout()[2]
    bufs = [e.alloc(max(n, 16)) for n in (nv * ns, nv * pitch, nv * 48, nv * 2 * p * 8)]
    d_raw, d_lay, d_out, d_coef = bufs
    e.h2d(d_raw, codes)
    e.layout(hpgv.LAYOUT_ASSOC, d_raw, ns, nv, d_lay)
    e.sync()
    e.h2d(d_out, np.full(nv * 48, 0xAB, np.uint8))
    e.assoc_linear_dev(d_lay, nv, d_out, d_coef if coef else None, stream=stream)
    e.sync(stream)
    out = e.d2h(d_out, (nv,), hpgv.LINEAR_RESULT)
    cf = e.d2h(d_coef, (nv, 2, p), np.float64) if coef else None
    for b in bufs:
        e.free(b)
    return out, cf


def same(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("key", ln.CASES, ids=ln.case_id)
def test_the_three_entry_points_against_the_oracle(key):
    case, exp = ln.expectations(*key)
    n_all = len(case["gt"])
    e = engine(case)
    out, cf = run_dev(e, case)
    worst = 0.0
    for x in exp:
        r = x["row"]
        worst = max(worst, ln.check_row(out[r], cf[r], x, (key, r, x["name"])))
    print("%s: worst deviation %.3g standard errors, tolerance %.3g" % (ln.case_id(key), worst, ln.DEVICE_TOL))
    if ln.well_sized(*key):
        assert (out["status"][:ln.N_ROWS] == ln.OK).sum() >= 0.9 * ln.N_ROWS
    # d_coef NULL: the same records; the host batch and the text: the same records and coefficients, bit for bit
    plain, none = run_dev(e, case, coef=False)
    assert same(plain, out) and none is None
    hb, hc = e.assoc_linear(case["gt"], coef=True)
    assert same(hb, out) and same(hc, cf)
    assert same(e.assoc_linear(case["gt"]), out)
    rt = e.assoc_linear_text(ln.text_of(case["gt"]), coef=True)
    assert rt["n_lines"] == n_all and not rt["status"].any()
    assert same(rt["out"], out) and same(rt["coef"], cf)
    if "exact_row" in case:                               # y = 3 + 2 d on that row's observations
        r = case["exact_row"]
        cls = ln.classify(case["gt"][r, case["coh"]])
        e.set_phenotype(case["y_exact"])
        o2, c2 = run_dev(e, case, slice(r, r + 1))
        if (cls <= 2).sum() > 2 and len(set(cls[cls <= 2])) > 1:
            ln.check_exact(o2[0], c2[0], key)
    e.close()


def test_rows_longer_than_one_step_of_the_correction_scan():
    """1 300 cohort columns: the scan for flagged positions takes 1 024 positions per step, so these rows need a second one, and
    their mostly_missing row several batches of 64 in both steps"""
    key = (700, 600, 3, "unit")
    case, exp = ln.expectations(*key)
    e = engine(case)
    assert e.assoc_layout()[2] > 1024
    out, cf = e.assoc_linear(case["gt"], coef=True)
    worst = max(ln.check_row(out[x["row"]], cf[x["row"]], x, (key, x["row"], x["name"])) for x in exp)
    print("%s: worst deviation %.3g standard errors, tolerance %.3g" % (ln.case_id(key), worst, ln.DEVICE_TOL))
    assert sum(x["kind"] == "ok" for x in exp) >= 70
    e.close()


@pytest.mark.parametrize("key", [(37, 29, 3, "unit"), (129, 70, 13, "unit"), (300, 211, 14, "unit"), (15, 17, 0, "unit"), (129, 70, 9, "unit")],
                         ids=ln.case_id)
def test_split_calls_and_repeated_runs_are_bit_identical(key):
    case, _ = ln.expectations(*key)
    n_all = len(case["gt"])
    e = engine(case)
    whole, wc = run_dev(e, case)
    again, ac = run_dev(e, case)
    assert same(whole, again) and same(wc, ac)
    at = 0
    for nv in (1, 5, 15, 16, 17, n_all - 54):               # pieces that start and end inside a tile of 16 rows, then the rest
        part, pc = run_dev(e, case, slice(at, at + nv))
        assert same(part, whole[at:at + nv]) and same(pc, wc[at:at + nv]), (at, nv)
        at += nv
    assert at == n_all
    e.close()


def test_a_stream_of_the_callers():
    case, _ = ln.expectations(64, 64, 3, "unit")
    e = engine(case)
    ref, rc = run_dev(e, case)
    s = C.c_void_p()
    assert e.L.hpgv_stream_create(e.h, C.byref(s)) == hpgv.OK
    got, gc = run_dev(e, case, stream=s)
    assert e.L.hpgv_stream_destroy(e.h, s) == hpgv.OK
    assert same(got, ref) and same(gc, rc)
    e.close()


def test_the_image_follows_the_set_calls_in_either_order():
    case, exp = ln.expectations(37, 29, 3, "unit")
    e = engine(case)
    ref, rc = run_dev(e, case)
    e.close()
    e = engine(case, order="cohort,phenotype,covariates")       # the covariates after the phenotype: the same image
    got, gc = run_dev(e, case)
    assert same(got, ref) and same(gc, rc)
    cov = case["cov"].copy()
    y = case["y"].copy()
    cov[case["cond"] == 2] = 123.0                         # OTHER columns: any value, the same records
    y[case["cond"] == 2] = np.inf
    e.set_covariates(cov)
    e.set_phenotype(y)
    assert same(run_dev(e, case)[0], ref)
    # without covariates: C = 0, the (37, 29, 0)-shaped fit on the same rows and the same trait
    e.set_covariates(None)
    base, bc = run_dev(e, case, C_=0)
    assert bc.shape == (len(case["gt"]), 2, 2) and not same(base, ref)
    for r in range(0, ln.N_ROWS, 5):
        cls, yy, _ = ln.cohort_view(case, r)
        o = ln.ref_fit(cls, yy)
        ln.check_row(base[r], bc[r], dict(kind="ok", ref=o), r)
    e.set_covariates(case["cov"])
    assert same(run_dev(e, case)[0], ref)
    # another trait: other records; the first one again: the first records
    e.set_phenotype(np.where(case["cond"] == 2, 0.0, case["y"] * 2.0 + 1.0))
    twice, _ = run_dev(e, case)
    ok = ref["status"] == ln.OK
    assert np.allclose(twice["beta"][ok], 2.0 * ref["beta"][ok], rtol=1e-9, atol=1e-12) and np.allclose(twice["stat"][ok], ref["stat"][ok], rtol=1e-8)
    e.set_phenotype(case["y"])
    assert same(run_dev(e, case)[0], ref)
    e.close()


def test_a_new_cohort_clears_the_phenotype():
    case, _ = ln.expectations(37, 29, 3, "unit")
    e = engine(case)
    ref = e.assoc_linear(case["gt"])
    L, p = e.L, hpgv._ptr
    out = np.zeros(len(case["gt"]), hpgv.LINEAR_RESULT)
    gt = case["gt"]
    e.set_cohort(case["cond"])                             # the same cohort set again: the phenotype is gone all the same
    assert L.hpgv_assoc_linear(e.h, p(gt), gt.shape[1], len(gt), p(out), None) == hpgv.ERR_STATE
    assert b"hpgv_set_phenotype" in L.hpgv_last_error(e.h)
    e.set_phenotype(case["y"])                             # C = 0 now: the covariates went with the cohort
    assert not same(e.assoc_linear(gt), ref)
    e.set_covariates(case["cov"])
    assert same(e.assoc_linear(gt), ref)
    e.set_phenotype(None)                                  # cleared by the caller
    assert L.hpgv_assoc_linear(e.h, p(gt), gt.shape[1], len(gt), p(out), None) == hpgv.ERR_STATE
    e.close()


def test_a_group_context_gives_every_member_the_phenotype():
    case, _ = ln.expectations(37, 29, 3, "unit")
    e = engine(case)
    ref, rc = e.assoc_linear(case["gt"], coef=True)
    e.close()
    g = hpgv.Engine([0, 0])
    g.set_cohort(case["cond"])
    g.set_phenotype(case["y"])
    g.set_covariates(case["cov"])
    text = ln.text_of(case["gt"])
    for _ in range(3):                                     # dealt to either member
        out, cf = g.assoc_linear(case["gt"], coef=True)
        assert same(out, ref) and same(cf, rc)
        assert same(g.assoc_linear_text(text)["out"], ref)
    assert same(run_dev(g.member(1), case)[0], ref)       # the second member's own state, through its *_dev call
    g.close()


def test_error_codes():
    case, _ = ln.expectations(15, 17, 1, "unit")
    L = hpgv.load()
    e = hpgv.Engine(0)
    n = len(case["cond"])
    y = np.ascontiguousarray(np.nan_to_num(case["y"]))
    p = hpgv._ptr
    out = np.zeros(4, hpgv.LINEAR_RESULT)
    gt = np.ascontiguousarray(case["gt"][:4])
    nl = C.c_int(0)
    # before a cohort
    assert L.hpgv_set_phenotype(e.h, p(y), n) == hpgv.ERR_STATE
    assert L.hpgv_assoc_linear(e.h, p(gt), n, 4, p(out), None) == hpgv.ERR_STATE
    assert L.hpgv_assoc_linear_dev(e.h, None, 0, None, None, None) == hpgv.ERR_STATE
    assert L.hpgv_assoc_linear_text(e.h, b"", 0, 0, C.byref(nl), None, None, None, None, None) == hpgv.ERR_STATE
    e.set_cohort(case["cond"])
    # a cohort, no phenotype
    assert L.hpgv_assoc_linear(e.h, p(gt), n, 4, p(out), None) == hpgv.ERR_STATE
    assert L.hpgv_assoc_linear_dev(e.h, None, 0, None, None, None) == hpgv.ERR_STATE
    assert L.hpgv_assoc_linear_text(e.h, b"", 0, 0, C.byref(nl), None, None, None, None, None) == hpgv.ERR_STATE
    assert L.hpgv_set_phenotype(e.h, p(y), n - 1) == hpgv.ERR_INVALID
    assert L.hpgv_set_phenotype(e.h, p(y), n + 1) == hpgv.ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        y2 = y.copy()
        y2[case["coh"][3]] = bad                           # a cohort column
        assert L.hpgv_set_phenotype(e.h, p(y2), n) == hpgv.ERR_INVALID
        assert b"not finite" in L.hpgv_last_error(e.h)
    assert L.hpgv_assoc_linear(e.h, p(gt), n, 4, p(out), None) == hpgv.ERR_STATE      # a refused phenotype sets none
    y2 = y.copy()
    y2[case["cond"] == 2] = np.inf                         # OTHER columns may hold anything
    assert L.hpgv_set_phenotype(e.h, p(y2), n) == hpgv.OK
    assert L.hpgv_set_phenotype(e.h, None, 0) == hpgv.OK           # clears, whatever n_samples says
    assert L.hpgv_assoc_linear_dev(e.h, None, 0, None, None, None) == hpgv.ERR_STATE
    assert L.hpgv_set_phenotype(e.h, p(y), n) == hpgv.OK
    d = e.alloc(4096)
    odd = C.c_void_p(d.value + 8)
    assert L.hpgv_assoc_linear_dev(e.h, odd, 1, d, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_linear_dev(e.h, d, 1, odd, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_linear_dev(e.h, d, 1, d, C.c_void_p(d.value + 4), None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_linear_dev(e.h, d, -1, d, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_linear_dev(e.h, None, 1, d, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_linear_dev(e.h, d, 1, None, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_linear_dev(e.h, None, 0, None, None, None) == hpgv.OK
    assert L.hpgv_assoc_linear(e.h, p(gt), n - 1, 4, p(out), None) == hpgv.ERR_INVALID      # pitch below n_samples
    assert L.hpgv_assoc_linear(e.h, None, n, 4, p(out), None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_linear(e.h, p(gt), n, 4, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_linear(e.h, p(gt), n, -1, p(out), None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_linear(e.h, None, n, 0, None, None) == hpgv.OK
    assert L.hpgv_assoc_linear_text(e.h, b"x\n", 2, 1, None, None, None, None, p(out), None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_linear_text(e.h, b"x\n", 2, 1, C.byref(nl), None, None, None, None, None) == hpgv.ERR_INVALID
    assert L.hpgv_assoc_linear_text(e.h, b"x\n", 2, -1, C.byref(nl), None, None, None, p(out), None) == hpgv.ERR_INVALID
    e.free(d)
    e.close()
