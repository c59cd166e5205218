"""The stratified association on the host (hpgv_cmh_fit: the function the statistics kernel compiles), the within file's reader
and the runner's refusals -- no GPU.  hpgv_cmh_fit against the oracles of cmh_golden on hand tables and random tables for
K in {1, 2, 9, 70}; the NaN rules; the identities of a common odds ratio, of the fitted counts and of relabelled strata."""
import math
import os
from decimal import Decimal

import numpy as np
import pytest

import cmh_golden as cg
from helpers import TOL, assert_close, assert_p_close, close, hpgv

STRATA = [1, 2, 9, 70]


def _check(tab, what=""):
    got, exp = hpgv.cmh_fit(tab), cg.fit(tab)
    assert int(got["n_strata_cmh"]) == exp["n_strata_cmh"] and int(got["n_strata_bd"]) == exp["n_strata_bd"], what
    for k in cg.FIELDS:
        (assert_p_close if k in ("p", "p_bd") else assert_close)(float(got[k]), exp[k], "%s %s" % (what, k))
        assert not math.isinf(float(got[k])), (what, k)
    return got, exp


def _random_tables(rng, K, scale):
    t = rng.integers(0, scale, (K, 4)).astype(np.int32)
    t[rng.random(K) < 0.15] = 0                                       # empty strata
    t[rng.random(K) < 0.1, rng.integers(0, 4)] = 0                    # a zero cell
    return t


def test_hand_tables():
    # two strata, checked by hand: E = 30 * 40 / 75 + 12 * 14 / 51, V = 30 * 45 * 40 * 35 / (75^2 * 74) + 12 * 39 * 14 * 37 / (51^2 * 50)
    tab = np.array([[10, 20, 30, 15], [5, 7, 9, 30]], np.int32)
    got, exp = _check(tab, "hand")
    E = 30 * 40 / 75 + 12 * 14 / 51
    V = 30 * 45 * 40 * 35 / (75 ** 2 * 74) + 12 * 39 * 14 * 37 / (51 ** 2 * 50)
    assert close(float(got["chisq"]), (15 - E) ** 2 / V)
    assert close(float(got["or_mh"]), (10 * 15 / 75 + 5 * 30 / 51) / (20 * 30 / 75 + 7 * 9 / 51))
    assert int(got["n_strata_cmh"]) == 2 and int(got["n_strata_bd"]) == 2
    assert float(got["l95"]) < float(got["or_mh"]) < float(got["u95"])


@pytest.mark.parametrize("K", STRATA)
def test_random_tables(K):
    rng = np.random.default_rng(100 + K)
    some_bd = 0
    for trial in range(40):
        tab = _random_tables(rng, K, (3, 12, 60, 2000)[trial % 4])
        got, _ = _check(tab, "K=%d trial %d" % (K, trial))
        some_bd += not math.isnan(float(got["chisq_bd"]))
    assert some_bd >= (0 if K == 1 else 10)                           # the Breslow-Day comparison says something


@pytest.mark.parametrize("K", STRATA)
def test_a_common_odds_ratio(K):
    """a d = 2 b c in every stratum: OR_MH is 2 exactly, the fitted counts are the observed ones, CHISQ_BD is 0 within TOL"""
    tab = cg.common_or_tables(np.random.default_rng(200 + K), K)
    got, exp = _check(tab, "common")
    assert float(got["or_mh"]) == 2.0
    if K == 1:
        assert math.isnan(float(got["chisq_bd"])) and math.isnan(float(got["p_bd"])) and int(got["n_strata_bd"]) == 1      # df < 1
    else:
        assert abs(float(got["chisq_bd"])) <= TOL and int(got["n_strata_bd"]) == K
        assert close(float(got["p_bd"]), 1.0)
        for k, A in exp["fitted"]:                                    # the oracle's own fitted counts are the observed ones
            assert abs(A - int(tab[k, 0])) < Decimal(10) ** -40


@pytest.mark.parametrize("K", [2, 9, 70])
def test_the_fitted_counts_reproduce_the_odds_ratio_and_the_margins(K):
    rng = np.random.default_rng(300 + K)
    checked = 0
    for _ in range(10):
        tab = _random_tables(rng, K, 60)
        exp = cg.fit(tab)
        if not exp["fitted"]:
            continue
        psi = Decimal(exp["or_mh"])                                   # (the f64 of the exact ratio: 1e-16 off)
        for k, A in exp["fitted"]:
            a, b, c, d = (int(x) for x in tab[k])
            m1, m0, n1 = a + b, c + d, a + c
            assert max(0, n1 - m0) <= A <= min(m1, n1)
            fit_or = A * (m0 - n1 + A) / ((m1 - A) * (n1 - A))        # the fitted table has the margins by construction
            assert abs(fit_or / psi - 1) < Decimal(10) ** -14
            checked += 1
    assert checked >= 10


@pytest.mark.parametrize("K", [2, 9, 70])
def test_relabelling_the_strata(K):
    rng = np.random.default_rng(400 + K)
    for _ in range(10):
        tab = _random_tables(rng, K, 60)
        a, b = hpgv.cmh_fit(tab), hpgv.cmh_fit(tab[rng.permutation(K)])
        assert a["n_strata_cmh"] == b["n_strata_cmh"] and a["n_strata_bd"] == b["n_strata_bd"]
        for k in cg.FIELDS:
            assert_close(float(b[k]), float(a[k]), k)


def test_nan_rules():
    nan = math.isnan
    f = lambda rows: hpgv.cmh_fit(np.array(rows, np.int32))
    mono = f([[8, 0, 12, 0], [3, 0, 5, 0]])                           # monomorphic: every V is 0
    assert nan(mono["chisq"]) and nan(mono["p"]) and nan(mono["or_mh"]) and nan(mono["se"]) and nan(mono["chisq_bd"]) and nan(mono["p_bd"])
    assert mono["n_strata_cmh"] == 2 and mono["n_strata_bd"] == 0
    missing = f([[0, 0, 0, 0], [0, 0, 0, 0]])                         # all calls missing
    assert nan(missing["chisq"]) and nan(missing["or_mh"]) and missing["n_strata_cmh"] == 0 and missing["n_strata_bd"] == 0
    none = hpgv.cmh_fit(np.zeros((0, 4), np.int32))                   # no stratum at all
    assert nan(none["chisq"]) and none["n_strata_cmh"] == 0
    small = f([[1, 0, 0, 0], [3, 2, 4, 5], [2, 3, 1, 4]])             # a stratum with n < 2 takes no part
    rest = f([[3, 2, 4, 5], [2, 3, 1, 4]])
    assert small["n_strata_cmh"] == 2 and small["n_strata_bd"] == 2
    for k in cg.FIELDS:
        assert float(small[k]) == float(rest[k]), k
    aff = f([[4, 6, 0, 0], [3, 2, 4, 5], [2, 3, 1, 4]])               # a stratum with only affected samples: E = a, V = 0
    assert aff["n_strata_cmh"] == 3 and aff["n_strata_bd"] == 2
    assert_close(float(aff["chisq"]), float(rest["chisq"]), "chisq")
    assert float(aff["or_mh"]) == float(rest["or_mh"])
    no_s = f([[3, 0, 4, 5], [2, 3, 0, 4]])                            # b c == 0 everywhere: sum S == 0
    assert not nan(no_s["chisq"]) and nan(no_s["or_mh"]) and nan(no_s["se"]) and nan(no_s["l95"]) and nan(no_s["u95"]) and nan(no_s["chisq_bd"])
    no_r = f([[0, 3, 4, 5], [2, 3, 4, 0]])                            # a d == 0 everywhere: sum R == 0
    assert not nan(no_r["chisq"]) and nan(no_r["or_mh"]) and nan(no_r["chisq_bd"])
    one = f([[3, 2, 4, 5], [4, 0, 2, 0]])                             # one stratum enters Breslow-Day: df < 1
    assert one["n_strata_bd"] == 1 and not nan(one["or_mh"]) and nan(one["chisq_bd"]) and nan(one["p_bd"])
    for r in (mono, missing, small, aff, no_s, no_r, one):
        assert not any(math.isinf(float(r[k])) for k in cg.FIELDS)
    with pytest.raises(hpgv.HpgvError) as err:
        f([[1, -1, 2, 3]])
    assert err.value.code == hpgv.ERR_INVALID


def test_the_tails_against_scipy_where_it_is_installed():
    stats = pytest.importorskip("scipy.stats")
    for df in (1, 2, 3, 4, 7, 8, 19, 69, 70):
        for x in (0.0, 1e-3, 0.5, 1.0, 3.3, 17.0, 80.0, 300.0):
            want = float(stats.chi2.sf(x, df))
            if df > 1 or want > 1e-6:                                 # (the 1-df tail is 1 - P: its digits end near 1e-16)
                assert abs(cg.tail(x, df) - want) <= 1e-12 * max(want, 1e-300) + 1e-300, (df, x)


def test_the_breslow_day_tail_through_the_fit():
    """p_bd for even and odd df, small and large: tables built so that chisq_bd is large"""
    rng = np.random.default_rng(5)
    seen = set()
    for K in (2, 3, 4, 9, 10, 70):
        for scale in (30, 400):
            tab = rng.integers(1, scale, (K, 4)).astype(np.int32)
            tab[::2, 0] *= 3                                          # heterogeneous odds ratios
            got, exp = _check(tab, "K=%d" % K)
            assert int(got["n_strata_bd"]) == K and not math.isnan(float(got["p_bd"]))
            seen.add((K - 1) % 2)
    assert seen == {0, 1}


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def test_within_read(tmp_path):
    names = ["S3", "S1", "S7", "S2", "S9"]
    good = _write(tmp_path / "within.txt", "FID IID CLUSTER\nf1 S1 north\nf2\tS2\tsouth\n\nf3 S3  south\nf7 S7 east\nfx nobody west\n")
    st, k = hpgv.within_read(good, names)
    assert k == 3 and st.tolist() == [0, 1, 2, 0, -1]                 # south, north, east by first appearance in the order of names; S9 has no line
    st, k = hpgv.within_read(good, names, take=[0, 1, 1, 1, 1])       # S3 not taken: north comes first
    assert k == 3 and st.tolist() == [-1, 0, 1, 2, -1]
    st, k = hpgv.within_read(_write(tmp_path / "nohdr.txt", "a S1 7\nb S2 7\n"), names)
    assert k == 1 and st.tolist() == [-1, 0, -1, 0, -1]
    bad = {"short": "a S1 x\nb S2\n", "two_columns": "a S1\nb S2\n", "dup": "a S1 x\nb S1 y\n", "ragged": "a S1 x\nb S2 y z\n",
           "many": "".join("f S%d c%d\n" % (i, i) for i in range(hpgv.CMH_MAX_STRATA + 1))}
    for name, text in bad.items():
        with pytest.raises(hpgv.HpgvError) as err:
            hpgv.within_read(_write(tmp_path / ("bad_%s.txt" % name), text), names)
        assert err.value.code == hpgv.ERR_INVALID, name
    edge = _write(tmp_path / "edge.txt", "".join("f S%d c%d\n" % (i, i) for i in range(hpgv.CMH_MAX_STRATA)))
    assert hpgv.within_read(edge, names)[1] == 5
    for path in (None, str(tmp_path / "missing.txt")):
        with pytest.raises(hpgv.HpgvError) as err:
            hpgv.within_read(path, names)
        assert err.value.code == hpgv.ERR_INVALID


def test_the_runner_refuses_bad_arguments_before_the_engine_starts(tmp_path):
    vcf, ped = _write(tmp_path / "in.vcf", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"), _write(tmp_path / "ped.txt", "f S1 0 0 1 2\n")
    within = _write(tmp_path / "within.txt", "f S1 a\n")
    bad = {"short": "a S1\n", "dup": "a S1 x\nb S1 y\n", "many": "".join("f S%d c%d\n" % (i, i) for i in range(hpgv.CMH_MAX_STRATA + 1))}
    out = str(tmp_path / "refused.cmh")
    calls = [(None, ped, within, out), (vcf, None, within, out), (vcf, ped, None, out), (vcf, ped, within, None), (vcf, ped, str(tmp_path / "missing.txt"), out)]
    calls += [(vcf, ped, _write(tmp_path / ("bad_%s.txt" % n), t), out) for n, t in bad.items()]
    for args in calls:
        with pytest.raises(hpgv.HpgvError) as err:
            hpgv.run_assoc_cmh(*args)
        assert err.value.code == hpgv.ERR_INVALID, args
        assert not os.path.exists(out), args
