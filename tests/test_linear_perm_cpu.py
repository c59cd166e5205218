"""The host side of the permutations of the linear statistic (include/hpgv.h "permutations of the linear statistic"): the order
shuffle against its documented generator, hpgv_linear_perm_fit against the extended-precision oracle of linear_perm_golden on every
case, T_obs of complete rows against hpgv_linear_fit's statistic, the error codes -- and what the GPU tests rely on: the yardstick
E_PERM still covers the closed form, no row lies near the take-part rule, and the oracle leaves no pair undecided, so the counts
the device must give are equalities."""
import ctypes as C

import numpy as np
import pytest

import linear_perm_golden as lp
from helpers import hpgv


def test_the_yardstick_covers_the_closed_form():
    e = lp.measure_E()
    print("E_perm measured %.3g, constant %.3g; host tolerance %.3g, device tolerance %.3g" % (e, lp.E_PERM, lp.HOST_TOL, lp.DEVICE_TOL))
    assert e <= lp.E_PERM
    assert lp.HOST_TOL == max(4 * lp.E_PERM, 1e-12) and lp.DEVICE_TOL == max(64 * lp.E_PERM, 1e-12)


@pytest.mark.parametrize("key", lp.CASES, ids=lp.case_id)
def test_the_oracle_decides_every_pair_and_every_row(key):
    case, exp = lp.expectations(*key)
    r = exp["ratio"]
    assert not np.any((r > 1e-16) & (r < 1e-6)), "a row near the rule D <= 1e-12 sw2"
    names = case["names"]
    for name, part in zip(names, exp["part"][lp.N_ROWS:]):
        want = name in ("single_het", "missing_gt_observed", "missing_last_of_segments") and sum(key[:2]) - (key[2] + 2) >= 1
        assert bool(part) == want or (want and sum(key[:2]) < 17), (name, part)         # (five columns: such a row may have no spread)
    assert np.all(np.isnan(exp["t_obs"]) == ~exp["part"]) and np.all(np.isnan(exp["T"]) == ~exp["part"][:, None])
    if key not in lp.COUNT_CASES:
        return
    assert sum(key[:2]) >= 17 and not np.any(np.all(case["order"] == np.arange(case["order"].shape[1]), axis=1))
    assert exp["part"][:lp.N_ROWS].all()
    for rows, n_perms in ((slice(None), lp.N_PERMS), (slice(0, 17), 129), (slice(16, 17), 17), (slice(None), 1)):
        c = lp.counts(exp, rows, n_perms)
        assert c["undecided"] == 0 and c["undecided_max"] == 0, (rows, n_perms, c["undecided"], c["undecided_max"])


def test_order_shuffle_rows_are_bijections_of_the_cohort():
    rng = np.random.default_rng(5)
    cond = rng.integers(0, 3, 211).astype(np.uint8)
    coh = np.flatnonzero(cond != 2)
    a = hpgv.perm_order_shuffle(cond, 40, 77)
    assert a.shape == (40, 211) and a.dtype == np.int32
    other = np.flatnonzero(cond == 2)
    assert np.all(a[:, other] == other)
    for row in a:
        assert sorted(row[coh]) == list(coh)
    assert len({row.tobytes() for row in a}) == 40
    # deterministic in (seed, p); row p does not depend on n_perms; another seed: other rows
    assert np.array_equal(hpgv.perm_order_shuffle(cond, 40, 77), a)
    assert np.array_equal(hpgv.perm_order_shuffle(cond, 7, 77), a[:7])
    assert not np.array_equal(hpgv.perm_order_shuffle(cond, 40, 78), a)
    assert np.array_equal(a, lp.order_shuffle(cond, 40, 77))
    # the walk is hpgv_perm_labels_shuffle's: the label a column gets is the label of the column whose residual it takes
    lab = hpgv.perm_labels_shuffle(cond, 40, 77)
    base = (cond == 1).astype(np.uint8)
    assert np.array_equal(lab[:, coh], base[a[:, coh]])


def test_order_shuffle_known_answer():
    """a 5-column cohort among 7 columns, seed 12345, written out from the documented generator (linear_perm_golden.order_shuffle)"""
    cond = np.array([1, 2, 0, 0, 1, 2, 1], np.uint8)
    want = [[4, 1, 0, 3, 6, 5, 2], [4, 1, 0, 3, 6, 5, 2], [4, 1, 3, 0, 2, 5, 6], [0, 1, 6, 2, 3, 5, 4]]
    assert lp.order_shuffle(cond, 4, 12345).tolist() == want
    assert hpgv.perm_order_shuffle(cond, 4, 12345).tolist() == want
    L = hpgv.load()
    out = np.zeros(7, np.int32)
    assert L.hpgv_perm_order_shuffle(None, 7, 1, 1, hpgv._ptr(out)) == hpgv.ERR_INVALID
    assert L.hpgv_perm_order_shuffle(hpgv._ptr(cond), 7, 1, 1, None) == hpgv.ERR_INVALID
    assert L.hpgv_perm_order_shuffle(hpgv._ptr(cond), -1, 1, 1, hpgv._ptr(out)) == hpgv.ERR_INVALID
    assert L.hpgv_perm_order_shuffle(hpgv._ptr(cond), 7, -1, 1, hpgv._ptr(out)) == hpgv.ERR_INVALID
    assert L.hpgv_perm_order_shuffle(hpgv._ptr(cond), 7, 0, 1, None) == hpgv.OK


@pytest.mark.parametrize("key", lp.CASES, ids=lp.case_id)
def test_the_host_fit_against_the_oracle(key):
    case, exp = lp.expectations(*key)
    cls, y, cov, order = lp.cohort_view(case)
    long = sum(key[:2]) > 1000
    worst = 0.0
    for r in range(len(cls)):
        od = order[:33] if long and r % 8 else order            # (a long cohort: every permutation on one row in eight)
        t_obs, t_perm = hpgv.linear_perm_fit(cls[r], y, cov if key[2] else None, od)
        dev = max(lp.deviation(t_obs, exp["t_obs"][r]), lp.deviation(t_perm, exp["T"][r, :len(od)]))
        assert dev <= lp.HOST_TOL, (key, r, dev)
        worst = max(worst, dev)
    print("%s: worst deviation %.3g, tolerance %.3g" % (lp.case_id(key), worst, lp.HOST_TOL))


@pytest.mark.parametrize("key", [(15, 17, 0, "unit"), (37, 29, 3, "unit"), (129, 70, 14, "unit"), (300, 211, 3, "mean1000")], ids=lp.case_id)
def test_t_obs_of_a_complete_row_is_the_linear_fits_statistic(key):
    """Frisch-Waugh-Lovell: without a missing call the imputed row is the row"""
    case, exp = lp.expectations(*key)
    cls, y, cov, order = lp.cohort_view(case)
    n = 0
    for r in range(len(cls)):
        if np.any(cls[r] > 2) or not exp["part"][r]:
            continue
        rec, _ = hpgv.linear_fit(cls[r], y, cov if key[2] else None)
        t_obs, _ = hpgv.linear_perm_fit(cls[r], y, cov if key[2] else None, order[:1])
        assert rec["status"] == hpgv.LINEAR_OK and rec["df"] == len(y) - key[2] - 2
        assert abs(t_obs - rec["stat"]) <= 1e-9 * max(1.0, abs(rec["stat"])), (r, t_obs, rec["stat"])
        n += 1
    assert n >= 20


def test_host_fit_error_codes():
    L, p = hpgv.load(), hpgv._ptr
    n, C_ = 20, 2
    rng = np.random.default_rng(3)
    cls = rng.integers(0, 3, n).astype(np.uint8)
    y, cov = rng.standard_normal(n), np.ascontiguousarray(rng.standard_normal((n, C_)))
    order = np.ascontiguousarray(np.stack([rng.permutation(n) for _ in range(3)]).astype(np.int32))
    t_obs, t_perm = np.zeros(1), np.zeros(3)
    ok = lambda **k: L.hpgv_linear_perm_fit(k.get("cls", p(cls)), k.get("y", p(y)), k.get("cov", p(cov)), k.get("n", n), k.get("C", C_),
                                            k.get("order", p(order)), k.get("np", 3), k.get("t_obs", p(t_obs)), k.get("t_perm", p(t_perm)))
    assert ok() == hpgv.OK and np.all(np.isfinite(t_perm))
    for bad in (dict(cls=None), dict(y=None), dict(cov=None), dict(order=None), dict(t_obs=None), dict(t_perm=None), dict(n=-1), dict(C=-1),
                dict(C=hpgv.LOGISTIC_MAX_COVAR + 1), dict(np=-1)):
        assert ok(**bad) == hpgv.ERR_INVALID, bad
    assert ok(np=0, order=None, t_perm=None) == hpgv.OK
    for v in (np.nan, np.inf):
        y2 = y.copy(); y2[4] = v
        assert ok(y=p(y2)) == hpgv.ERR_INVALID
        c2 = cov.copy(); c2[4, 1] = v
        assert ok(cov=p(c2)) == hpgv.ERR_INVALID
    for bad_row in ([0] * n, list(range(1, n)) + [n], [-1] + list(range(1, n))):
        o2 = order.copy(); o2[1] = bad_row
        assert ok(order=p(o2)) == hpgv.ERR_INVALID, bad_row
    c2 = cov.copy(); c2[:, 1] = 3.0 * c2[:, 0] - 1.0            # collinear covariates
    assert ok(cov=p(c2)) == hpgv.ERR_INVALID
    c2 = cov.copy(); c2[:, 0] = 7.0                            # a constant one: collinear with the intercept
    assert ok(cov=p(c2)) == hpgv.ERR_INVALID
    # df < 1: NaN everywhere
    assert L.hpgv_linear_perm_fit(p(cls), p(y), p(cov), 4, C_, p(np.ascontiguousarray(np.tile(np.arange(4, dtype=np.int32), (3, 1)))), 3, p(t_obs), p(t_perm)) == hpgv.OK
    assert np.isnan(t_obs[0]) and np.all(np.isnan(t_perm))
