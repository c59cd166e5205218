"""Trend permutation (the PERM_TREND form of k_assoc_perm, csrc/hpgv_assoc_perm_kernels.h): the permuted sums {R_p, D_p} off the
matrix cores bit-exact against numpy's valid @ y and dosage @ y, n_ge and batch_max exact against the engine's own statistics
kernel run on the permuted class tables (and within TOL of the exact rational trend statistic), splitting, the label state, and
the allelic form on the same engine and labels unchanged."""
import functools

import numpy as np
import pytest

import model_golden as mg
from helpers import TOL, assert_close, hpgv

pytestmark = pytest.mark.gpu

WIDTHS = [(2, 3), (37, 45), (64, 64), (301, 412)]      # (affected, unaffected): 5 columns; two ragged k-steps; whole chunks; 12 k-steps, the last ragged
VARIANTS = [1, 17, 150]                                 # one row; a ragged 16-row tile; three workgroups, the last ragged
PERMS = [1, 5, 33, 100]                                 # below one 16-column tile; ragged tiles
CASES = [(w, nv, P, (i + j + k) % 2 == 0) for i, w in enumerate(WIDTHS) for j, nv in enumerate(VARIANTS) for k, P in enumerate(PERMS)]


def _expected(chi, t_obs):
    """n_ge and batch_max of a [nv, P] statistic matrix by the NaN rules"""
    with np.errstate(invalid="ignore"):
        n_ge = (chi >= t_obs[:, None]).sum(axis=1).astype(np.int32)
    bmax = np.fmax.reduce(chi, axis=0, initial=0.0) if chi.shape[0] else np.zeros(chi.shape[1])
    return n_ge, bmax


@functools.lru_cache(maxsize=None)
def _reference(width, nv, n_perms, quirks, special=()):
    """of a case: the sums [nv, P, 2] from numpy, then (n_ge, batch_max, t_obs) from the engine's statistics kernel on the
    permuted class tables (r_k from numpy, s_k = n_k - r_k) and the exact rational statistic [nv, P]"""
    c = mg.case(width, nv, n_perms, quirks, special=special)
    valid, dosage = mg.classes(c["strict"])
    y = (c["labels"] * (c["cond"] != 2)).astype(np.int64)                  # [P, ns]: columns outside the cohort take no part
    sums = np.stack([valid.astype(np.int64) @ y.T, dosage @ y.T], axis=2).astype(np.int32)
    r = np.stack([((valid & (dosage == k)).astype(np.int64) @ y.T) for k in range(3)], axis=2)       # [nv, P, 3]
    n = (c["c8"][:, 0:3] + c["c8"][:, 3:6]).astype(np.int64)
    tables = np.zeros((nv, n_perms, 8), np.int32)
    tables[:, :, 0:3], tables[:, :, 3:6] = r, n[:, None, :] - r
    e = hpgv.Engine(0)
    chi = mg.stats_dev(e, tables.reshape(-1, 8))[:, mg.TREND].reshape(nv, n_perms)
    t_obs = mg.stats_dev(e, c["c8"])[:, mg.TREND]
    e.close()
    N, W1, W2 = n.sum(axis=1), n[:, 1] + 2 * n[:, 2], n[:, 1] + 4 * n[:, 2]
    exact = mg.trend_exact(N[:, None], W1[:, None], W2[:, None], sums[:, :, 0].astype(np.int64), sums[:, :, 1].astype(np.int64))
    return (sums,) + _expected(chi, t_obs) + (t_obs, exact)


@pytest.mark.parametrize("width,nv,n_perms,quirks", CASES)
def test_sums_and_statistics(width, nv, n_perms, quirks):
    c = mg.case(width, nv, n_perms, quirks)
    sums, exp_ge, exp_max, t_obs, exact = _reference(width, nv, n_perms, quirks)
    e = mg.engine(c)
    got = mg.run_dev(e, c, perm=True)
    e.close()
    c8 = got["counts8"]
    assert np.array_equal(c8, c["c8"])
    assert np.array_equal(got["sums"], sums)
    assert np.array_equal(got["sums"][:, 0, 0], c8[:, 0:3].sum(axis=1))              # row 0 is the observed labelling: (R, D)
    assert np.array_equal(got["sums"][:, 0, 1], c8[:, 1] + 2 * c8[:, 2])
    assert np.array_equal(got["n_ge"], exp_ge)
    assert np.array_equal(mg.bits(got["batch_max"]), mg.bits(exp_max))
    assert np.array_equal(mg.bits(got["chisq5"][:, mg.TREND]), mg.bits(t_obs))
    assert np.all(got["n_ge"][np.isnan(t_obs)] == 0)
    if nv >= 3:
        assert np.isnan(t_obs[1]) and np.isnan(t_obs[2])
    assert_close(got["batch_max"], np.fmax.reduce(exact, axis=0, initial=0.0), "batch_max", TOL)
    assert not np.isinf(got["batch_max"]).any()


MID = ((37, 45), 150, 33, True)


def test_splitting_the_variants_merges_by_maximum():
    c = mg.case(*MID)
    _, exp_ge, exp_max, _, _ = _reference(*MID)
    e = mg.engine(c)
    parts = [mg.run_dev(e, c, rows, perm=True) for rows in (slice(0, 50), slice(50, 51), slice(51, 150))]
    empty = mg.run_dev(e, c, slice(0, 0), perm=True)
    e.close()
    assert np.array_equal(np.concatenate([p["n_ge"] for p in parts]), exp_ge)
    assert np.array_equal(mg.bits(np.maximum.reduce([p["batch_max"] for p in parts])), mg.bits(exp_max))
    assert not empty["batch_max"].any()                  # no variants: the identity of the merge


def test_label_state():
    c = mg.case(*MID)
    _, exp_ge, exp_max, _, _ = _reference(*MID)
    e = hpgv.Engine(0)
    e.set_cohort(c["cond"])
    d = e.alloc(4096)
    dev_call = lambda: e.L.hpgv_assoc_trend_perm_dev(e.h, d, 0, d, d, d, None, None)
    assert dev_call() == hpgv.ERR_STATE
    with pytest.raises(hpgv.HpgvError, match="hpgv error %d" % hpgv.ERR_STATE):
        e.assoc_model(c["codes"], perm=True)
    e.set_perm_labels(c["labels"])
    for _ in range(2):                                   # the labels survive consecutive calls
        res = e.assoc_model(c["codes"], perm=True)
        assert np.array_equal(res["n_ge"], exp_ge) and np.array_equal(mg.bits(res["batch_max"]), mg.bits(exp_max))
    e.set_perm_labels(None)                              # n_perms == 0 drops them
    assert dev_call() == hpgv.ERR_STATE
    e.set_perm_labels(c["labels"])
    assert dev_call() == hpgv.OK
    e.set_cohort(c["cond"])                              # so does a new cohort
    assert dev_call() == hpgv.ERR_STATE
    e.close()


def test_the_allelic_form_is_unchanged_beside_it():
    """hpgv_assoc_perm on the same engine and labels, after a trend call: its counts and chi-square are hpgv_assoc's, and its n_ge
    and batch_max what the chi-square kernel gives on the permuted allele tables"""
    c = mg.case(*MID)
    e = mg.engine(c)
    e.assoc_model(c["codes"], perm=True)
    res = e.assoc_perm(c["codes"])
    ref = e.assoc(hpgv.TASK_CHISQ, c["codes"])
    for k in ("A1", "A2", "U1", "U2", "odds", "chisq", "p"):
        assert np.array_equal(res[k], ref[k], equal_nan=True), k
    valid, dosage = mg.classes(c["strict"])
    y = (c["labels"] * (c["cond"] != 2)).astype(np.int64)
    a1 = (valid * (2 - dosage)) @ y.T                    # reference alleles of the labelled samples
    a2 = dosage @ y.T
    R1, R2 = (ref["A1"] + ref["U1"]).astype(np.int64), (ref["A2"] + ref["U2"]).astype(np.int64)
    tables = np.stack([a1, a2, R1[:, None] - a1, R2[:, None] - a2], axis=2).astype(np.int32).reshape(-1, 4)
    n = len(tables)
    d_c, d_o, d_x, d_p = e.alloc(n * 16), e.alloc(n * 8), e.alloc(n * 8), e.alloc(n * 8)
    e.h2d(d_c, tables)
    e.assoc_chisq(d_c, n, d_o, d_x, d_p)
    e.sync()
    chi = e.d2h(d_x, (n,), np.float64).reshape(c["nv"], c["n_perms"])
    e.close()
    exp_ge, exp_max = _expected(chi, ref["chisq"])
    assert np.array_equal(res["n_ge"], exp_ge) and np.array_equal(mg.bits(res["batch_max"]), mg.bits(exp_max))
