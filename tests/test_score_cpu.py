"""Allele scoring without a device (include/hpgv.h "Score"): hpgv_score_table against the numpy definition on hand-made rows, the
limbs, hpgv_score_frac_bits, the quantisation bound against math.fsum of the unquantised terms, and the row-range plan."""
import math

import numpy as np
import pytest

import ibs_golden as ig
import score_golden as sg
from helpers import hpgv
from model_golden import classes

INT_MIN = -2 ** 31


@pytest.fixture(scope="module", autouse=True)
def built():
    hpgv.build()


def _check_rows(c4, w, s, flags, impute):
    used, lim, c = hpgv.score_table(c4, w, s, flags, impute)
    eu, qg, qm, ec = sg.row_terms(c4, w, s, flags, impute)
    assert np.array_equal(used, eu), (used, eu)
    assert np.array_equal(lim[:, :, :4].astype(np.int64), sg.limbs(qg)) and np.array_equal(lim[:, :, 4:].astype(np.int64), sg.limbs(qm))
    assert np.array_equal(c, ec)
    # the limbs recombine to the integers and lie in their ranges
    place = np.array([1, 256, 65536, 1 << 24], np.int64)
    assert np.array_equal((lim[:, :, :4].astype(np.int64) * place).sum(axis=-1), qg)
    assert np.array_equal((lim[:, :, 4:].astype(np.int64) * place).sum(axis=-1), qm)
    assert np.abs(lim[:, :, 3]).max(initial=0) <= 64 and np.abs(lim[:, :, 7]).max(initial=0) <= 64
    assert np.abs(qg).max(initial=0) <= 2 ** 30 and np.abs(qm).max(initial=0) <= 2 ** 30 and np.abs(ec).max(initial=0) <= 2 ** 30
    return used, qg, qm, ec


def test_table_on_hand_made_rows():
    # class counts: p = 0, 1, 0.5, an odd frequency, T = 0, a negative count
    counts = [(10, 0, 0, 0), (0, 0, 7, 1), (3, 4, 3, 0), (5, 0, 5, 2), (17, 5, 1, 3), (0, 0, 0, 9), (-1, 2, 2, 0), (1, 0, 0, 0)]
    weights = [(0.75, -1.25, 3.0), (1e-3, 123.456, -0.5), (0.0, 1.0, -1.0), (2.5, 0.5, 1.5), (-7.0, 0.1, 0.3)]
    for s in ([0, 4, 20], [-2, 0, 1], [25, 10, -3]):
        for impute in (0, 1):
            for fl in (0, sg.FLIP, sg.SKIP, sg.SKIP | sg.FLIP):
                c4 = np.array([c for c in counts for _ in weights], np.int32)
                w = np.array([x for _ in counts for x in weights], np.float64)
                used, qg, qm, c = _check_rows(c4, w, s, np.full(len(c4), fl, np.uint8), impute)
                assert used.any() == ((fl & sg.SKIP) == 0) and not used[c4[:, :3].sum(axis=1) <= 0].any() and not used[c4[:, 0] < 0].any()
                if fl == sg.FLIP and not impute:
                    # a flipped missing byte without imputation contributes c + qm = 0 exactly
                    assert np.array_equal(c + qm, np.zeros_like(c)) and c.any()
                if fl == 0 and not impute:
                    assert not qm.any() and not c.any()


def test_q_at_the_limit_ties_and_negative_frac_bits():
    c4 = np.array([[3, 4, 3, 0]], np.int32)
    for fl in (0, sg.FLIP):
        for impute in (0, 1):
            fa = np.array([fl], np.uint8)
            # |q| exactly 2^28 is used, the next integer up is not
            for w, s, ok in ((2.0 ** 28, 0, True), (2.0 ** 28 + 1, 0, False), (-(2.0 ** 28), 0, True), (1.0, 28, True), (1.0 + 2.0 ** -27, 28, False),
                             (2.0 ** 28 + 0.5, 0, True), (2.0 ** 28 + 0.75, 0, False), (2.0 ** 40, -12, True), (2.0 ** 40 + 2.0 ** 13, -12, False)):
                used, qg, _, _ = _check_rows(c4, [[w]], [s], fa, impute)
                assert bool(used[0]) == ok, (w, s)
                if ok:
                    assert abs(int(qg[0, 0])) == 2 ** 28
            # ties go to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> 0, -1.5 -> -2
            used, qg, _, _ = _check_rows(np.repeat(c4, 5, axis=0), [[0.5], [1.5], [2.5], [-0.5], [-1.5]], [0], np.repeat(fa, 5), impute)
            assert used.all() and np.array_equal(np.abs(qg[:, 0]), [0, 2, 2, 0, 2])
            # a negative frac_bits: 1000 at s = -3 is 125; 1004 is 125.5 -> 126 (even), 1012 is 126.5 -> 126
            used, qg, _, _ = _check_rows(np.repeat(c4, 3, axis=0), [[1000.0], [1004.0], [1012.0]], [-3], np.repeat(fa, 3), impute)
            assert np.array_equal(np.abs(qg[:, 0]), [125, 126, 126])
    # one weight of a row out of range, or not finite, makes the whole row unused
    for bad in (2.0 ** 29, float("nan"), float("inf"), -float("inf")):
        used, lim, c = hpgv.score_table(c4, [[1.0, bad, 2.0]], [0, 0, 0], [0], 1)
        assert not used[0] and not lim.any() and not c.any()
        _check_rows(c4, [[1.0, bad, 2.0]], [0, 0, 0], [0], 1)
    # refusals of the host function: a frac_bits out of range, n_scores out of range
    assert not hpgv.score_table(c4, [[1.0]], [901], [0], 1)[0][0] and not hpgv.score_table(c4, [[1.0]], [-901], [0], 1)[0][0]
    assert not hpgv.score_table(c4, [[1.0]], [900], [0], 1)[0][0] and hpgv.score_table(c4, [[2.0 ** -880]], [900], [0], 1)[0][0]
    assert not hpgv.score_table(c4, np.ones((1, 33)), np.zeros(33, np.int32), [0], 1)[0][0]


def test_frac_bits():
    fb = hpgv.score_frac_bits
    assert fb(0.0) == 0 and fb(-0.0) == 0
    for bad in (float("nan"), float("inf"), -float("inf"), -1.0, -1e-300):
        assert fb(bad) == INT_MIN
    for e in (-40, -1, 0, 1, 5, 27, 28, 29, 100):
        x = 2.0 ** e
        assert fb(x) == 28 - (e + 1) and fb(np.nextafter(x, 0.0)) == 28 - e and fb(np.nextafter(x, np.inf)) == 28 - (e + 1)
    assert fb(5e-324) == 900 and fb(2.2250738585072014e-308) == 900 and fb(2.0 ** -873) == 900 and fb(2.0 ** -872) == 899
    assert fb(1.7976931348623157e308) == -900 and fb(2.0 ** 927) == -900 and fb(2.0 ** 926) == -899
    # no weight at or below the maximum makes a row unused, and the maximum itself uses at least 27 bits
    rng = np.random.default_rng(12)
    mags = np.abs(rng.standard_normal(1000)) * 10.0 ** rng.integers(-30, 31, 1000)
    c4 = np.array([[3, 4, 3, 1]] * 4, np.int32)
    for m in mags:
        s = fb(m)
        w = np.array([[m], [-m], [np.nextafter(m, 0.0)], [m * rng.random()]])
        used, qg, _, _ = sg.row_terms(c4, w, [s], np.array([0, sg.FLIP, 0, sg.FLIP], np.uint8), 1)
        assert used.all() and 2 ** 27 <= abs(int(qg[0, 0])) <= 2 ** 28
    used, _, _ = hpgv.score_table(np.repeat(c4[:1], 1000, axis=0), mags[:, None], [fb(mags.max())], np.zeros(1000, np.uint8), 1)
    assert used.all()


def _exact_terms(codes, w, flags, class4, used, impute):
    """per (score, column) the list of unquantised f64 terms of the used rows"""
    valid, g = classes(codes)
    rows, cols = codes.shape
    T = 2.0 * class4[:, :3].sum(axis=1)
    with np.errstate(all="ignore"):
        p = (class4[:, 1] + 2.0 * class4[:, 2]) / T
    flip = (flags & sg.FLIP) != 0
    dose = np.where(valid, np.where(flip[:, None], 2 - g, g).astype(np.float64),
                    (np.where(flip, 2.0 * (1.0 - p), 2.0 * p) if impute else np.zeros(rows))[:, None])
    return np.where(used[:, None], dose, 0.0)


@pytest.mark.parametrize("impute", [0, 1])
def test_quantisation_bound(impute):
    """|value - exact| <= n_used 2^-s + one ulp of the result: each used row moves a column's value by at most 2^-s (the header's
    bound), and exact is math.fsum of the unquantised terms w x dosage (each product rounded once: half an ulp of a term, far
    below 2^-s at the frac_bits of hpgv_score_frac_bits, which leaves at least 27 bits above 2^-s and a term has 53)."""
    rows, cols, ns = 300, 130, 3
    codes = ig.matrix(rows, cols)
    w, s, flags = sg.random_inputs(rows, ns, 77)
    G = sg.golden(codes, w, s, flags, impute)
    val = sg.value(G["acc"], G["const"], s)
    dose = _exact_terms(codes, w, flags, G["class4"], G["used"], impute)
    n_used = int(G["const"][ns])
    assert n_used > rows // 2
    for k in range(ns):
        for j in range(cols):
            exact = math.fsum((w[:, k] * dose[:, j]).tolist())
            tol = n_used * 2.0 ** -int(s[k]) + np.spacing(abs(exact))
            assert abs(val[k, j] - exact) <= tol, (k, j, val[k, j], exact, tol)


def test_plan_rows():
    plan, cap = hpgv.score_plan_rows, 1 << 22
    for nv in (0, 1, 63, 64, 65, 300, 5000, 65536, 4_000_000, cap - 1, cap, cap + 1, cap + 192, 3 * cap + 5, 2 ** 31 - 1):
        for nc in (1, 20, 200, 10_000, 50_000):
            for ns in (1, 8, 32):
                for cus in (1, 256, 304):
                    per = plan(nv, nc, ns, cus)
                    assert per % 64 == 0 and 64 <= per <= cap
                    ranges = -(-nv // per) if nv else 0
                    assert ranges * per >= nv                                  # the ranges cover the rows
                    if nv > cap:
                        assert ranges >= 2
                    if ranges >= 2:
                        # equal ranges: the last is short by less than 64 rows per range
                        assert nv - (ranges - 1) * per > per - 64 * ranges
    # few columns, many rows: the ranges fill the device; many columns, few rows: the tiles do
    assert -(-4_000_000 // plan(4_000_000, 200, 4, 256)) * 4 >= 256
    assert -(-50_000 // 64) * -(-3000 // plan(3000, 50_000, 4, 256)) >= 256
    assert plan(cap + 192, 20, 1, 256) < cap
