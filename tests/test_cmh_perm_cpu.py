"""The host side of the permutation within strata (include/hpgv.h "Permutation within strata"), no device needed:
hpgv_perm_labels_shuffle_within, hpgv_cmh_fit's chisq held to the bit patterns recorded before the CMH sums were factored out of
it for the permutation kernel (tests/golden/cmh_fit_chisq_bits.json), and the runner's refusals."""
import json
import os

import numpy as np
import pytest

import cmh_golden as cg
import cmh_perm_golden as pg
from helpers import hpgv


def _cohort(rng, ns=60):
    cond = rng.permutation(np.array([1] * 22 + [0] * 30 + [2] * (ns - 52), np.uint8))
    stratum = rng.integers(0, 4, ns).astype(np.int32)
    stratum[rng.permutation(np.flatnonzero(cond != 2))[:5]] = -1      # five cohort columns in no stratum
    stratum[stratum == 2] = 11                                        # the numbers need not be dense
    return cond, stratum


def test_every_row_keeps_each_stratums_affected_count():
    cond, stratum = _cohort(np.random.default_rng(1))
    rows = hpgv.perm_labels_shuffle_within(cond, stratum, 40, 1234)
    assert rows.shape == (40, len(cond)) and rows.max() == 1
    cohort = cond != 2
    for k in np.unique(stratum[cohort & (stratum >= 0)]):
        m = cohort & (stratum == k)
        assert (rows[:, m].sum(axis=1) == (cond[m] == 1).sum()).all(), k
    out = cohort & (stratum < 0)
    assert (rows[:, out] == (cond[out] == 1)).all()                   # in no stratum: the observed label
    assert not rows[:, ~cohort].any()                                 # HPGV_COND_OTHER: 0
    assert len({r.tobytes() for r in rows}) > 30                      # and they are shuffles
    big = cohort & (stratum == 0)
    assert (rows[:, big] != (cond[big] == 1)).any()


def test_a_row_does_not_depend_on_the_number_of_rows_and_follows_the_seed():
    cond, stratum = _cohort(np.random.default_rng(2))
    three, nine = hpgv.perm_labels_shuffle_within(cond, stratum, 3, 99), hpgv.perm_labels_shuffle_within(cond, stratum, 9, 99)
    assert np.array_equal(three, nine[:3])
    assert not np.array_equal(nine, hpgv.perm_labels_shuffle_within(cond, stratum, 9, 100))
    assert hpgv.perm_labels_shuffle_within(cond, stratum, 0, 99).shape == (0, len(cond))


def test_one_stratum_of_everyone_is_the_plain_shuffle():
    """with the whole cohort in one stratum the walk and the draws are hpgv_perm_labels_shuffle's"""
    cond, _ = _cohort(np.random.default_rng(3))
    assert np.array_equal(hpgv.perm_labels_shuffle_within(cond, np.zeros(len(cond), np.int32), 7, 5), hpgv.perm_labels_shuffle(cond, 7, 5))


def test_the_shuffle_refuses_bad_arguments():
    cond, stratum = _cohort(np.random.default_rng(4))
    L, out = hpgv.load(), np.zeros((2, len(cond)), np.uint8)
    p = hpgv._ptr
    assert L.hpgv_perm_labels_shuffle_within(p(cond), p(stratum), len(cond), 2, 1, p(out)) == hpgv.OK
    assert L.hpgv_perm_labels_shuffle_within(None, p(stratum), len(cond), 2, 1, p(out)) == hpgv.ERR_INVALID
    assert L.hpgv_perm_labels_shuffle_within(p(cond), None, len(cond), 2, 1, p(out)) == hpgv.ERR_INVALID
    assert L.hpgv_perm_labels_shuffle_within(p(cond), p(stratum), len(cond), 2, 1, None) == hpgv.ERR_INVALID
    assert L.hpgv_perm_labels_shuffle_within(p(cond), p(stratum), -1, 2, 1, p(out)) == hpgv.ERR_INVALID
    assert L.hpgv_perm_labels_shuffle_within(p(cond), p(stratum), len(cond), -1, 1, p(out)) == hpgv.ERR_INVALID


def test_cmh_fit_is_bit_identical_to_the_recorded_patterns():
    with open(os.path.join(os.path.dirname(__file__), "golden", "cmh_fit_chisq_bits.json")) as f:
        rec = json.load(f)["cases"]
    assert len(rec) >= 6
    seen_nan = 0
    for r in rec:
        c = cg.case(tuple(r["width"]), r["nv"], r["K"], quirks=r["quirks"])
        got = pg.fit_chisq(c["tables"]).view(np.uint64)
        want = np.array([int(b, 16) for b in r["chisq_bits"]], np.uint64)
        assert np.array_equal(got, want), (r["width"], r["nv"], r["K"])
        seen_nan += int(np.isnan(want.view(np.float64)).sum())
    assert seen_nan >= 6


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def test_the_runner_refuses_bad_arguments_before_the_engine_starts(tmp_path):
    vcf, ped = _write(tmp_path / "in.vcf", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"), _write(tmp_path / "ped.txt", "f S1 0 0 1 2\n")
    within = _write(tmp_path / "within.txt", "f S1 a\n")
    out = str(tmp_path / "refused.cmh")
    calls = [(None, ped, within, out, 5), (vcf, None, within, out, 5), (vcf, ped, None, out, 5), (vcf, ped, within, None, 5),
             (vcf, ped, within, out, 0), (vcf, ped, within, out, -3), (vcf, ped, str(tmp_path / "missing.txt"), out, 5),
             (vcf, ped, _write(tmp_path / "bad_short.txt", "a S1\n"), out, 5)]
    for args in calls:
        with pytest.raises(hpgv.HpgvError) as err:
            hpgv.run_assoc_cmh_perm(*args, seed=1)
        assert err.value.code == hpgv.ERR_INVALID, args
        assert not os.path.exists(out) and not os.path.exists(out + ".mperm"), args
