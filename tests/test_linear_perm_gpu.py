"""The permutations of the linear statistic on the device (include/hpgv.h "permutations of the linear statistic"): k_linear_perm_rows
and k_linear_perm through hpgv_assoc_linear_perm_dev, the host-batch and the text entry points against the extended-precision
oracle of linear_perm_golden -- t_obs and every T_p(v) under its device tolerance, n_ge and the EMP2 ranks as equalities (the CPU
suite asserts that the oracle leaves no pair undecided) -- over cohorts that need several wave stripes and k-steps, 0 to 14
covariates, row counts and permutation counts on either side of a tile; then bit identity of split calls and repeated runs, a stream
of the caller's, the permutations' life with the set calls, a group context and the error codes."""
import ctypes as C

import numpy as np
import pytest

import linear_perm_golden as lp
from helpers import hpgv

pytestmark = pytest.mark.gpu

GPU_CASES = ([(nA, nU, C_, "unit") for nA, nU in [(15, 17), (129, 70), (300, 211)] for C_ in (0, 1, 13, 14)]
             + [lp.LONG + (3, "unit"), (300, 211, 3, "mean1000")])


def engine(case, n_perms=lp.N_PERMS, dev=0):
    e = hpgv.Engine(dev)
    nA, nU, _ = e.set_cohort(case["cond"])
    assert (nA, nU) == (case["nA"], case["nU"])
    if case["C"]:
        e.set_covariates(case["cov"])
    e.set_phenotype(case["y"])
    if n_perms:
        e.set_linear_perms(case["order"][:n_perms])
    return e


def run_dev(e, case, rows=slice(None), n_perms=lp.N_PERMS, perm_t=True, stream=None):
    """layout and the two kernels on device buffers: dict(t_obs, n_ge, batch_max, perm_t or None)"""
    codes = np.ascontiguousarray(case["gt"][rows])
    nv, ns = codes.shape
    pitch = e.assoc_layout()[2]
    bufs = [e.alloc(max(n, 16)) for n in (nv * ns, nv * pitch, nv * 8, nv * 4, n_perms * 8, nv * n_perms * 8)]
    d_raw, d_lay, d_t, d_ge, d_max, d_pt = bufs
    e.h2d(d_raw, codes)
    e.layout(hpgv.LAYOUT_ASSOC, d_raw, ns, nv, d_lay)
    e.sync()
    for d, n in ((d_t, nv * 8), (d_ge, nv * 4), (d_max, n_perms * 8), (d_pt, nv * n_perms * 8)):
        e.h2d(d, np.full(n, 0xAB, np.uint8))
    e.assoc_linear_perm_dev(d_lay, nv, d_t, d_ge, d_max, d_pt if perm_t else None, stream=stream)
    e.sync(stream)
    out = dict(t_obs=e.d2h(d_t, (nv,), np.float64), n_ge=e.d2h(d_ge, (nv,), np.int32), batch_max=e.d2h(d_max, (n_perms,), np.float64),
               perm_t=e.d2h(d_pt, (nv, n_perms), np.float64) if perm_t else None)
    for b in bufs:
        e.free(b)
    return out


def same(a, b):
    return a.tobytes() == b.tobytes()


def same_run(a, b, perm_t=True):
    return all(same(a[k], b[k]) for k in ("t_obs", "n_ge", "batch_max") + (("perm_t",) if perm_t else ()))


def check(got, exp, rows=slice(None), n_perms=lp.N_PERMS, where=""):
    """a run against the oracle; returns the largest deviation"""
    want = lp.counts(exp, rows, n_perms)
    dev = lp.deviation(got["t_obs"], exp["t_obs"][rows])
    if got["perm_t"] is not None:
        dev = max(dev, lp.deviation(got["perm_t"], exp["T"][rows, :n_perms]))
    dmax = lp.deviation(got["batch_max"], want["batch_max"])
    print("%s: t deviation %.3g, maxima %.3g, tolerance %.3g" % (where, dev, dmax, lp.DEVICE_TOL))
    assert dev <= lp.DEVICE_TOL and dmax <= lp.DEVICE_TOL, (where, dev, dmax)
    assert want["undecided"] == 0 and want["undecided_max"] == 0
    assert np.array_equal(got["n_ge"], want["n_ge"]), where
    assert np.all(got["batch_max"] >= 0.0) and np.all((got["batch_max"] == 0.0) == (want["batch_max"] == 0.0))
    t = np.abs(exp["t_obs"][rows])
    e1, e2 = hpgv.perm_pvalues(np.abs(got["t_obs"]), got["n_ge"], got["batch_max"])
    w1, w2 = hpgv.perm_pvalues(t, want["n_ge"], want["batch_max"])
    assert np.array_equal(e1, w1, equal_nan=True) and np.array_equal(e2, w2, equal_nan=True), where
    return max(dev, dmax)


@pytest.mark.parametrize("key", GPU_CASES, ids=lp.case_id)
def test_the_three_entry_points_against_the_oracle(key):
    case, exp = lp.expectations(*key)
    n_all = len(case["gt"])
    e = engine(case)
    got = run_dev(e, case)
    check(got, exp, where=lp.case_id(key))
    assert np.all(np.isnan(got["t_obs"]) == ~exp["part"]) and np.all(got["n_ge"][~exp["part"]] == 0)
    # d_perm_t NULL: the same outputs; the host batch and the text: the same, bit for bit, with hpgv_assoc_linear's records
    assert same_run(run_dev(e, case, perm_t=False), got, perm_t=False)
    rec = e.assoc_linear(case["gt"])
    hb = e.assoc_linear_perm(case["gt"])
    assert same_run(hb, got, perm_t=False) and same(hb["out"], rec)
    rt = e.assoc_linear_perm_text(lp.text_of(case["gt"]))
    assert rt["n_lines"] == n_all and not rt["status"].any()
    assert same_run(rt, got, perm_t=False) and same(rt["out"], rec)
    # Frisch-Waugh-Lovell: a row without a missing call has the regression's statistic
    full = np.flatnonzero(np.all(lp.classify(case["gt"][:, case["coh"]]) <= 2, axis=1) & exp["part"] & (rec["status"] == hpgv.LINEAR_OK))
    assert len(full) >= 20
    assert np.all(np.abs(got["t_obs"][full] - rec["stat"][full]) <= 1e-9 * np.maximum(1.0, np.abs(rec["stat"][full])))
    e.close()


@pytest.mark.parametrize("n_perms", [1, 16, 17, 129])
def test_row_counts_and_permutation_counts_on_either_side_of_a_tile(n_perms):
    key = (129, 70, 13, "unit")
    case, exp = lp.expectations(*key)
    e = engine(case)
    whole = run_dev(e, case)
    e.set_linear_perms(case["order"][:n_perms])
    for rows in (slice(5, 6), slice(16, 32), slice(50, 67), slice(None)):
        got = run_dev(e, case, rows, n_perms)
        # a permutation's column does not depend on how many follow it, a row not on its neighbours
        assert same(got["perm_t"], np.ascontiguousarray(whole["perm_t"][rows, :n_perms])) and same(got["t_obs"], whole["t_obs"][rows])
        check(got, exp, rows, n_perms, "%s rows %s perms %d" % (lp.case_id(key), rows, n_perms))
    e.close()


def test_a_cohort_of_five_columns_and_the_take_part_rules():
    case, exp = lp.expectations(0, 5, 3, "unit")             # df = 0: no row takes part
    e = engine(case, 17)
    got = run_dev(e, case, n_perms=17)
    assert np.all(np.isnan(got["t_obs"])) and np.all(np.isnan(got["perm_t"])) and not got["n_ge"].any() and not got["batch_max"].any()
    hb = e.assoc_linear_perm(case["gt"])
    assert same_run(hb, got, perm_t=False) and np.all(hb["out"]["status"] == hpgv.LINEAR_SINGULAR)
    e.close()
    for C_ in (0, 1):                                         # df = 3, 2: the statistics, and NaN for the rows the rules leave out
        case, exp = lp.expectations(0, 5, C_, "unit")
        e = engine(case, 33)
        got = run_dev(e, case, n_perms=33)
        assert max(lp.deviation(got["t_obs"], exp["t_obs"]), lp.deviation(got["perm_t"], exp["T"][:, :33])) <= lp.DEVICE_TOL
        assert np.all(got["n_ge"][~exp["part"]] == 0)
        e.close()
    # more covariates than the cohort has columns: collinear
    base = lp.ln.make_case(0, 5, 13)
    e = hpgv.Engine(0)
    e.set_cohort(base["cond"])
    e.set_covariates(base["cov"])
    e.set_phenotype(base["y"])
    order = np.ascontiguousarray(np.tile(np.arange(len(base["cond"]), dtype=np.int32), (2, 1)))
    assert e.L.hpgv_set_linear_perms(e.h, hpgv._ptr(order), 2) == hpgv.ERR_INVALID
    assert b"collinear" in e.L.hpgv_last_error(e.h)
    e.close()


@pytest.mark.parametrize("key", [(15, 17, 0, "unit"), (300, 211, 14, "unit"), lp.LONG + (3, "unit")], ids=lp.case_id)
def test_split_calls_and_repeated_runs_are_bit_identical(key):
    case, _ = lp.expectations(*key)
    n_all, n_perms = len(case["gt"]), 129
    e = engine(case, n_perms)
    whole = run_dev(e, case, n_perms=n_perms)
    assert same_run(run_dev(e, case, n_perms=n_perms), whole)
    at, bmax, n_ge = 0, np.zeros(n_perms), []
    for nv in (1, 5, 15, 16, 17, n_all - 54):               # pieces that start and end inside a tile of 16 and of 64 rows, then the rest
        part = run_dev(e, case, slice(at, at + nv), n_perms)
        assert same(part["perm_t"], np.ascontiguousarray(whole["perm_t"][at:at + nv])) and same(part["t_obs"], whole["t_obs"][at:at + nv]), (at, nv)
        bmax = np.maximum(bmax, part["batch_max"])
        n_ge.append(part["n_ge"])
        at += nv
    assert at == n_all
    assert same(bmax, whole["batch_max"]) and same(np.concatenate(n_ge), whole["n_ge"])       # batches merge by the element-wise maximum
    s = C.c_void_p()
    assert e.L.hpgv_stream_create(e.h, C.byref(s)) == hpgv.OK
    assert same_run(run_dev(e, case, n_perms=n_perms, stream=s), whole)
    assert e.L.hpgv_stream_destroy(e.h, s) == hpgv.OK
    e.close()


def test_the_set_calls_drop_the_permutations():
    case, _ = lp.expectations(15, 17, 1, "unit")
    e = engine(case, 17)
    ref = e.assoc_linear_perm(case["gt"])
    L, p, gt = e.L, hpgv._ptr, case["gt"]
    out, t_obs, n_ge, bmax = np.zeros(len(gt), hpgv.LINEAR_RESULT), np.zeros(len(gt)), np.zeros(len(gt), np.int32), np.zeros(17)
    call = lambda: L.hpgv_assoc_linear_perm(e.h, p(gt), gt.shape[1], len(gt), p(out), p(t_obs), p(n_ge), p(bmax))
    for drop in (lambda: e.set_phenotype(case["y"]), lambda: e.set_covariates(case["cov"]), lambda: e.set_linear_perms(None),
                 lambda: (e.set_cohort(case["cond"]), e.set_covariates(case["cov"]), e.set_phenotype(case["y"]))):
        assert call() == hpgv.OK
        drop()
        assert call() == hpgv.ERR_STATE and b"hpgv_set_linear_perms" in L.hpgv_last_error(e.h)
        assert L.hpgv_assoc_linear_perm_dev(e.h, None, 0, None, None, None, None, None) == hpgv.ERR_STATE
        e.set_linear_perms(case["order"][:17])
        assert same_run(e.assoc_linear_perm(gt), ref, perm_t=False)
    e.set_phenotype(None)                                  # no phenotype: no permutations can be set
    assert L.hpgv_set_linear_perms(e.h, p(case["order"]), 17) == hpgv.ERR_STATE
    e.close()


def test_a_group_context_gives_every_member_the_permutations():
    case, _ = lp.expectations(129, 70, 1, "unit")
    e = engine(case, 33)
    ref = e.assoc_linear_perm(case["gt"])
    e.close()
    g = engine(case, 33, dev=[0, 0])
    text = lp.text_of(case["gt"])
    for _ in range(3):                                     # dealt to either member
        assert same_run(g.assoc_linear_perm(case["gt"]), ref, perm_t=False)
        assert same_run(g.assoc_linear_perm_text(text), ref, perm_t=False)
    assert same_run(run_dev(g.member(1), case, n_perms=33), ref, perm_t=False)       # the second member's own state
    g.close()


def test_error_codes():
    case, _ = lp.expectations(15, 17, 1, "unit")
    L, p = hpgv.load(), hpgv._ptr
    e = hpgv.Engine(0)
    n = len(case["cond"])
    order = np.ascontiguousarray(case["order"][:4])
    gt = np.ascontiguousarray(case["gt"][:4])
    out, t_obs, n_ge, bmax = np.zeros(4, hpgv.LINEAR_RESULT), np.zeros(4), np.zeros(4, np.int32), np.zeros(4)
    nl = C.c_int(0)
    assert L.hpgv_set_linear_perms(e.h, p(order), 4) == hpgv.ERR_STATE                 # no cohort
    e.set_cohort(case["cond"])
    assert L.hpgv_set_linear_perms(e.h, p(order), 4) == hpgv.ERR_STATE                 # no phenotype
    e.set_covariates(case["cov"])
    e.set_phenotype(case["y"])
    assert L.hpgv_assoc_linear_perm(e.h, p(gt), n, 4, p(out), p(t_obs), p(n_ge), p(bmax)) == hpgv.ERR_STATE       # no permutations
    assert L.hpgv_assoc_linear_perm_text(e.h, b"", 0, 0, C.byref(nl), None, None, None, None, None, None, p(bmax)) == hpgv.ERR_STATE
    assert L.hpgv_set_linear_perms(e.h, None, 4) == hpgv.ERR_INVALID
    assert L.hpgv_set_linear_perms(e.h, p(order), -1) == hpgv.ERR_INVALID
    assert L.hpgv_set_linear_perms(e.h, p(order), (1 << 20) + 1) == hpgv.ERR_UNSUPPORTED
    coh = case["coh"]
    for j, v in ((coh[3], coh[4]), (coh[0], -1), (coh[1], n), (coh[2], int(np.flatnonzero(case["cond"] == 2)[0]))):
        bad = order.copy()
        bad[2, j] = v                                      # twice the same column, out of range, an OTHER column
        assert L.hpgv_set_linear_perms(e.h, p(bad), 4) == hpgv.ERR_INVALID
        assert b"row 2" in L.hpgv_last_error(e.h)
    other = order.copy()
    other[:, case["cond"] == 2] = -7                       # what a row holds in OTHER columns is not read
    assert L.hpgv_set_linear_perms(e.h, p(other), 4) == hpgv.OK
    assert L.hpgv_set_linear_perms(e.h, p(order), 4) == hpgv.OK
    assert L.hpgv_set_linear_perms(e.h, p(order), (1 << 20) + 1) == hpgv.ERR_UNSUPPORTED and L.hpgv_set_linear_perms(e.h, p(order), 4) == hpgv.OK
    e.set_linear_perms(order)
    d = e.alloc(4096)
    odd = C.c_void_p(d.value + 4)
    dev = L.hpgv_assoc_linear_perm_dev
    assert dev(e.h, C.c_void_p(d.value + 8), 1, d, d, d, None, None) == hpgv.ERR_INVALID
    assert dev(e.h, d, 1, odd, d, d, None, None) == hpgv.ERR_INVALID
    assert dev(e.h, d, 1, d, C.c_void_p(d.value + 2), d, None, None) == hpgv.ERR_INVALID
    assert dev(e.h, d, 1, d, d, odd, None, None) == hpgv.ERR_INVALID
    assert dev(e.h, d, 1, d, d, d, odd, None) == hpgv.ERR_INVALID
    assert dev(e.h, d, -1, d, d, d, None, None) == hpgv.ERR_INVALID
    assert dev(e.h, None, 1, d, d, d, None, None) == hpgv.ERR_INVALID
    assert dev(e.h, d, 1, None, d, d, None, None) == hpgv.ERR_INVALID
    assert dev(e.h, d, 1, d, None, d, None, None) == hpgv.ERR_INVALID
    assert dev(e.h, d, 1, d, d, None, None, None) == hpgv.ERR_INVALID
    assert dev(e.h, None, 0, None, None, None, None, None) == hpgv.ERR_INVALID        # batch_max is written even for no rows
    assert dev(e.h, None, 0, None, None, d, None, None) == hpgv.OK
    e.sync()
    assert not e.d2h(d, (4,), np.float64).any()
    call = L.hpgv_assoc_linear_perm
    assert call(e.h, p(gt), n - 1, 4, p(out), p(t_obs), p(n_ge), p(bmax)) == hpgv.ERR_INVALID      # pitch below n_samples
    assert call(e.h, None, n, 4, p(out), p(t_obs), p(n_ge), p(bmax)) == hpgv.ERR_INVALID
    assert call(e.h, p(gt), n, 4, None, p(t_obs), p(n_ge), p(bmax)) == hpgv.ERR_INVALID
    assert call(e.h, p(gt), n, 4, p(out), None, p(n_ge), p(bmax)) == hpgv.ERR_INVALID
    assert call(e.h, p(gt), n, 4, p(out), p(t_obs), None, p(bmax)) == hpgv.ERR_INVALID
    assert call(e.h, p(gt), n, 4, p(out), p(t_obs), p(n_ge), None) == hpgv.ERR_INVALID
    assert call(e.h, p(gt), n, -1, p(out), p(t_obs), p(n_ge), p(bmax)) == hpgv.ERR_INVALID
    bmax[:] = 9.0
    assert call(e.h, None, n, 0, None, None, None, p(bmax)) == hpgv.OK and not bmax.any()
    text = L.hpgv_assoc_linear_perm_text
    assert text(e.h, b"x\n", 2, 1, None, None, None, None, p(out), p(t_obs), p(n_ge), p(bmax)) == hpgv.ERR_INVALID
    assert text(e.h, b"x\n", 2, 1, C.byref(nl), None, None, None, None, p(t_obs), p(n_ge), p(bmax)) == hpgv.ERR_INVALID
    assert text(e.h, b"x\n", 2, 1, C.byref(nl), None, None, None, p(out), p(t_obs), p(n_ge), None) == hpgv.ERR_INVALID
    assert text(e.h, b"x\n", 2, -1, C.byref(nl), None, None, None, p(out), p(t_obs), p(n_ge), p(bmax)) == hpgv.ERR_INVALID
    # a line that is no record takes no part: NaN, no count, and it stays out of the maxima
    good = lp.text_of(case["gt"][:3])
    status = np.zeros(4, np.int32)
    lines = good.split(b"\n")
    mixed = b"\n".join([lines[0], b"not\ta\trecord", lines[1], lines[2], b""])
    assert text(e.h, mixed, len(mixed), 4, C.byref(nl), None, None, p(status), p(out), p(t_obs), p(n_ge), p(bmax)) == hpgv.OK
    ref = e.assoc_linear_perm(case["gt"][:3])
    assert nl.value == 4 and status[1] != 0 and not status[[0, 2, 3]].any()
    assert np.isnan(t_obs[1]) and n_ge[1] == 0 and same(t_obs[[0, 2, 3]], ref["t_obs"]) and same(n_ge[[0, 2, 3]], ref["n_ge"]) and same(bmax, ref["batch_max"])
    e.free(d)
    e.close()
