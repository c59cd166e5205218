"""The model tests (include/hpgv.h "model tests"): k_assoc_model_scan's class counts bit-exact against numpy, their identity with
the allelic scan's counts on the same laid-out rows, the five statistics of k_assoc_model_stats against an exact rational trend
statistic and explicit Pearson sums (cross-checked with corrcoef and scipy), and the host, text and group entry points against
the device chain."""
import numpy as np
import pytest

import model_golden as mg
from helpers import assert_close, assert_p_close, hpgv

pytestmark = pytest.mark.gpu

# (affected, unaffected): 5 columns; ragged chunks; whole chunks; 45 chunks; 101 chunks, a lane's second trip; 270 chunks, past the
# scan's tile of 4 x 64 chunks, so two tiles per row; no unaffected sample at all
WIDTHS = [(2, 3), (37, 45), (64, 64), (301, 412), (700, 900), (2100, 2200), (37, 0)]
VARIANTS = [1, 17, 150]                                 # one row; an odd count (the last wave has one row); many workgroups
CASES = [(w, nv, (i + j) % 2 == 0) for i, w in enumerate(WIDTHS) for j, nv in enumerate(VARIANTS)]


@pytest.mark.parametrize("width,nv,quirks", CASES)
def test_counts_and_statistics(width, nv, quirks):
    c = mg.case(width, nv, 0, quirks)
    mg.cross_check(c["strict"], c["cond"], c["c8"], c["chisq5"])
    e = mg.engine(c)
    got = mg.run_dev(e, c)
    e.close()
    c8 = got["counts8"]
    assert np.array_equal(c8, c["c8"])
    assert np.array_equal(c8[:, 6] + c8[:, 0:3].sum(axis=1), np.full(nv, width[0]))
    assert np.array_equal(c8[:, 7] + c8[:, 3:6].sum(axis=1), np.full(nv, width[1]))
    # the identity with the allelic scan on the same rows, and its chi-square bit for bit
    A1, A2, U1, U2 = got["counts4"].T
    assert np.array_equal(2 * c8[:, 0] + c8[:, 1], A1) and np.array_equal(c8[:, 1] + 2 * c8[:, 2], A2)
    assert np.array_equal(2 * c8[:, 3] + c8[:, 4], U1) and np.array_equal(c8[:, 4] + 2 * c8[:, 5], U2)
    assert np.array_equal(mg.bits(got["chisq5"][:, mg.ALLELIC]), mg.bits(got["chisq"]))
    # the five tests
    assert np.array_equal(np.isnan(got["chisq5"]), np.isnan(c["chisq5"]))
    assert np.array_equal(np.isnan(got["p5"]), np.isnan(c["chisq5"]))
    for t, name in enumerate(("geno", "trend", "allelic", "dom", "rec")):
        assert_close(got["chisq5"][:, t], c["chisq5"][:, t], "chisq " + name)
        assert_p_close(got["p5"][:, t], c["p5"][:, t], "p " + name)
    if nv >= 3:
        assert np.isnan(got["chisq5"][1:3]).all()           # all missing; monomorphic
        assert c8[1, 6] == width[0] and c8[1, 7] == width[1]


MID = ((37, 45), 150, 33, True)


def _same(a, b, keys=("counts8", "chisq5", "p5")):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.array_equal(mg.bits(a["chisq5"]), mg.bits(b["chisq5"])) and np.array_equal(mg.bits(a["p5"]), mg.bits(b["p5"]))


def test_host_and_text_entry_points():
    c = mg.case(*MID)
    e = mg.engine(c)
    dev = mg.run_dev(e, c, perm=True)
    assert np.array_equal(dev["counts8"], c["c8"])
    plain = e.assoc_model(c["codes"])                    # no permutation: no n_ge, no batch_max
    _same(plain, dev)
    assert "n_ge" not in plain
    res = e.assoc_model(c["codes"], perm=True)
    _same(res, dev)
    assert np.array_equal(res["n_ge"], dev["n_ge"]) and np.array_equal(mg.bits(res["batch_max"]), mg.bits(dev["batch_max"]))
    text = mg.text_of(c["codes"])
    rt = e.assoc_model_text(text, perm=True)
    assert rt["n_lines"] == c["nv"] and not rt["status"].any()
    _same(rt, dev)
    assert np.array_equal(rt["n_ge"], dev["n_ge"]) and np.array_equal(mg.bits(rt["batch_max"]), mg.bits(dev["batch_max"]))
    _same(e.assoc_model_text(text), dev)
    e.close()


def test_no_labels_are_needed_without_the_permutation():
    c = mg.case(*MID)
    e = mg.engine(c, labels=False)
    res = e.assoc_model(c["codes"])
    assert np.array_equal(res["counts8"], c["c8"])
    with pytest.raises(hpgv.HpgvError, match="hpgv error %d" % hpgv.ERR_STATE):
        e.assoc_model(c["codes"], perm=True)
    # exactly one of n_ge / batch_max
    gt = np.ascontiguousarray(c["codes"])
    out = [np.zeros((c["nv"], 8), np.int32), np.zeros((c["nv"], 5)), np.zeros((c["nv"], 5)), np.zeros(c["nv"], np.int32), np.zeros(64)]
    p = [hpgv._ptr(a) for a in out]
    assert e.L.hpgv_assoc_model(e.h, hpgv._ptr(gt), gt.shape[1], c["nv"], p[0], p[1], p[2], p[3], None) == hpgv.ERR_INVALID
    assert e.L.hpgv_assoc_model(e.h, hpgv._ptr(gt), gt.shape[1], c["nv"], p[0], p[1], p[2], None, p[4]) == hpgv.ERR_INVALID
    e.close()


def test_text_lines_that_are_no_records_take_no_part():
    c = mg.case(*MID)
    e = mg.engine(c)
    lines = mg.text_of(c["codes"]).split(b"\n")[:-1]
    keep = np.ones(c["nv"], bool)
    keep[[0, 40, 149]] = False
    text = b"".join((l if keep[i] else b"7\t5\trs") + b"\n" for i, l in enumerate(lines))      # three lines cut short
    rt = e.assoc_model_text(text, perm=True)
    sub = mg.run_dev(e, dict(c, codes=c["codes"][keep]), perm=True)
    e.close()
    assert rt["n_lines"] == c["nv"] and np.array_equal(rt["status"] != 0, ~keep)
    assert np.array_equal(rt["counts8"][keep], sub["counts8"]) and np.array_equal(mg.bits(rt["chisq5"][keep]), mg.bits(sub["chisq5"]))
    assert np.array_equal(rt["n_ge"][keep], sub["n_ge"]) and not rt["n_ge"][~keep].any()
    assert np.array_equal(mg.bits(rt["batch_max"]), mg.bits(sub["batch_max"]))


def test_group_context():
    c = mg.case(*MID)
    e = mg.engine(c)
    dev = mg.run_dev(e, c, perm=True)
    e.close()
    g = mg.engine(c, [0, 0])
    for _ in range(2):                                   # dealt to one member, then the other
        res = g.assoc_model(c["codes"], perm=True)
        _same(res, dev)
        assert np.array_equal(res["n_ge"], dev["n_ge"]) and np.array_equal(mg.bits(res["batch_max"]), mg.bits(dev["batch_max"]))
    rt = g.assoc_model_text(mg.text_of(c["codes"]), perm=True)
    _same(rt, dev)
    assert np.array_equal(rt["n_ge"], dev["n_ge"]) and np.array_equal(mg.bits(rt["batch_max"]), mg.bits(dev["batch_max"]))
    m = mg.run_dev(g.member(0), c, perm=True)
    _same(m, dev)
    assert np.array_equal(m["n_ge"], dev["n_ge"]) and np.array_equal(mg.bits(m["batch_max"]), mg.bits(dev["batch_max"]))
    g.close()
