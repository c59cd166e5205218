"""The host-only helpers of the label permutation (include/hpgv.h "label permutation, host side"): the label shuffle and the
empirical p-values.  No device: both are plain functions of libhpgv.so."""
import numpy as np
import pytest

from helpers import hpgv

COND = np.array([1, 0, 2, 1, 1, 0, 2, 0, 0, 1, 0, 2, 1, 0], np.uint8)      # 5 affected, 6 unaffected, 3 others, interleaved


def test_shuffle_keeps_the_affected_count_and_leaves_the_others_zero():
    lab = hpgv.perm_labels_shuffle(COND, 200, seed=7)
    assert lab.shape == (200, len(COND)) and lab.dtype == np.uint8
    assert set(np.unique(lab)) <= {0, 1}
    assert np.all(lab.sum(axis=1) == int((COND == 1).sum()))
    assert not lab[:, COND == 2].any()


def test_shuffle_is_deterministic_in_seed_and_row():
    a = hpgv.perm_labels_shuffle(COND, 64, seed=12345)
    b = hpgv.perm_labels_shuffle(COND, 64, seed=12345)
    assert np.array_equal(a, b)
    # row p depends on (seed, p) alone: a shorter matrix is a prefix of a longer one
    assert np.array_equal(hpgv.perm_labels_shuffle(COND, 10, seed=12345), a[:10])
    c = hpgv.perm_labels_shuffle(COND, 64, seed=12346)
    # 462 labellings of 11 columns with 5 ones: two of 64 rows agreeing by chance is common, all of them is not
    assert (a != c).any(axis=1).sum() > 32
    assert len({r.tobytes() for r in a}) > 32


def test_shuffle_is_uniform_over_the_cohort_columns():
    cond = np.array([1, 1, 1, 0, 0, 0, 0, 0, 0, 0], np.uint8)
    n, k, rows = len(cond), 3, 2000
    lab = hpgv.perm_labels_shuffle(cond, rows, seed=99)
    share = lab.mean(axis=0)
    # a column's label over independent rows is Bernoulli(k / n): the share's standard deviation is sqrt(p (1 - p) / rows)
    p = k / n
    sd = np.sqrt(p * (1 - p) / rows)
    assert np.all(np.abs(share - p) <= 5 * sd), share


def test_shuffle_degenerate_cohorts():
    assert hpgv.perm_labels_shuffle(np.array([2, 2], np.uint8), 3, seed=1).sum() == 0
    assert np.array_equal(hpgv.perm_labels_shuffle(np.array([1], np.uint8), 2, seed=1), [[1], [1]])
    assert hpgv.perm_labels_shuffle(COND, 0, seed=1).shape == (0, len(COND))


def _pvalues_by_definition(t_obs, n_ge, t_max):
    P = len(t_max)
    emp1 = (n_ge + 1.0) / (P + 1.0)
    with np.errstate(invalid="ignore"):
        emp2 = ((t_max[None, :] >= t_obs[:, None]).sum(axis=1) + 1.0) / (P + 1.0)
    nan = np.isnan(t_obs)
    emp1[nan] = np.nan
    emp2[nan] = np.nan
    return emp1, emp2


def test_pvalues_match_the_definitions():
    rng = np.random.default_rng(3)
    t_max = rng.chisquare(1, size=257) * 4.0          # unsorted
    t_max[10] = t_max[200] = 3.25                     # tied maxima
    t_obs = np.concatenate([rng.chisquare(1, size=40) * 5.0, [3.25, t_max[0], t_max.max(), t_max.min(), 0.0, 1e9, np.nan, np.nan]])
    n_ge = rng.integers(0, 258, size=len(t_obs)).astype(np.int32)
    emp1, emp2 = hpgv.perm_pvalues(t_obs, n_ge, t_max)
    exp1, exp2 = _pvalues_by_definition(t_obs, n_ge, t_max)
    assert np.array_equal(emp1, exp1, equal_nan=True)
    assert np.array_equal(emp2, exp2, equal_nan=True)
    # a tie counts: the variant whose statistic equals the largest maximum has exactly one permutation at or above it
    i = len(t_obs) - 6
    assert emp2[i] == 2.0 / 258.0
    assert emp2[len(t_obs) - 3] == 1.0 / 258.0        # above every maximum
    assert emp2[len(t_obs) - 4] == 1.0                # 0: every permutation is at or above


def test_pvalues_with_one_permutation():
    t_obs = np.array([1.0, 2.0, 3.0, np.nan])
    n_ge = np.array([1, 1, 0, 0], np.int32)
    emp1, emp2 = hpgv.perm_pvalues(t_obs, n_ge, np.array([2.0]))
    assert np.array_equal(emp1, [1.0, 1.0, 0.5, np.nan], equal_nan=True)
    assert np.array_equal(emp2, [1.0, 1.0, 0.5, np.nan], equal_nan=True)


def test_pvalues_refuse_no_permutations():
    with pytest.raises(hpgv.HpgvError):
        hpgv.perm_pvalues(np.array([1.0]), np.array([0], np.int32), np.zeros(0))
