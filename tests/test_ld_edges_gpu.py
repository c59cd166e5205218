"""The edge form of the LD band (include/hpgv.h "LD", hpgv_ld_edges_dev / hpgv_ld_edges): the list, sorted, must be the numpy
band's pairs with r2 >= min_r2 -- (a, b) exact, r2 bit for bit -- whatever the row width, the number of rows, the window and the
threshold; the counter is the true count whatever edge_cap is, and nothing is stored past edge_cap records."""
import ctypes as C

import numpy as np
import pytest

import clump_golden as cg
import ld_golden as lg
import model_golden as mg
from helpers import hpgv

pytestmark = pytest.mark.gpu

VARIANTS = [1, 2, 17, 65, 150, 300]
WINDOWS = [1, 63, 64, 100]
HIGH = 0.999


@pytest.fixture(scope="module")
def eng():
    e = lg.engine()
    yield e
    e.close()


def _thresholds(r2):
    return (0.0, cg.median_r2(r2), HIGH)


def test_goldens_are_neither_empty_nor_complete():
    """on the golden alone: per width a case whose edge set is a proper, non-empty part of the band, and planted pairs that
    reach the high threshold"""
    for width in lg.WIDTHS:
        r2 = lg.golden(width, 300, 64)[0]
        n = len(cg.edges_of_band(r2, cg.median_r2(r2)))
        assert 0 < n < np.isfinite(r2).sum()
        pr2 = cg.planted_golden(width, 300, 64)[0]
        ones, high = len(cg.edges_of_band(pr2, 1.0)), len(cg.edges_of_band(pr2, HIGH))
        assert ones >= 20 and high < np.isfinite(pr2).sum() // 4
        if width[0] >= 37:
            partial = cg.edges_of_band(pr2, 0.5)
            assert (partial["r2"] < HIGH).sum() >= 10             # the copies with redrawn bytes: high, below 1


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("nv", VARIANTS)
@pytest.mark.parametrize("width", lg.WIDTHS)
def test_set_equality(eng, width, nv, window):
    for what, codes, gold in (("random", lg.matrix(width, nv), lg.golden(width, nv, window)),
                              ("planted", cg.planted(width, nv), cg.planted_golden(width, nv, window))):
        laid = lg.lay(codes, width[0])
        for min_r2 in _thresholds(gold[0]):
            exp = cg.edges_of_band(gold[0], min_r2)
            got, count, guard_ok = cg.run_edges(eng, laid, window, min_r2)
            assert count == len(exp) and guard_ok, (what, min_r2, count, len(exp))
            cg.assert_edges_equal(got, exp, "%s, min_r2 %r" % (what, min_r2))


@pytest.mark.parametrize("window", [10, 100])
def test_b_begin(eng, window):
    width, nv = (37, 45), 300
    codes = cg.planted(width, nv)
    laid = lg.lay(codes, width[0])
    for b_begin in (37, 64, 299):
        r2 = lg.band(codes, window, b_begin=b_begin)[0]
        for min_r2 in (0.0, cg.median_r2(r2)):
            exp = cg.edges_of_band(r2, min_r2, b_begin=b_begin)
            got, count, guard_ok = cg.run_edges(eng, laid, window, min_r2, b_begin=b_begin)
            assert count == len(exp) and guard_ok and (b_begin == 299 or count > 0)
            cg.assert_edges_equal(got, exp, "b_begin %d" % b_begin)
    got, count, guard_ok = cg.run_edges(eng, laid, window, 0.0, b_begin=nv)               # nothing to do: the counter still zeroed
    assert count == 0 and len(got) == 0 and guard_ok


def test_skip_chromosomes_and_distances(eng):
    width, nv, window = (37, 45), 150, 20
    codes = cg.planted(width, nv)
    laid = lg.lay(codes, width[0])
    rng = np.random.default_rng(6)
    skip = (rng.random(nv) < 0.1).astype(np.uint8)
    skip[[15, 16, 64]] = 1
    chrom = np.where(np.arange(nv) < 40, 1, np.where(np.arange(nv) < 128, 2, 7)).astype(np.int32)
    pos = np.cumsum(rng.integers(0, 4, nv) * 50).astype(np.uint32) + 1000
    full = len(cg.edges_of_band(lg.band(codes, window)[0], 0.0))
    for kw in (dict(skip=skip), dict(chrom=chrom, pos=pos), dict(chrom=chrom, pos=pos, max_bp=500), dict(chrom=chrom, pos=pos, max_bp=499),
               dict(chrom=chrom, pos=pos, max_bp=0), dict(chrom=chrom, pos=pos, max_bp=350, skip=skip),
               dict(chrom=np.zeros(nv, np.int32), pos=pos[::-1].copy(), max_bp=200)):
        r2 = lg.band(codes, window, **kw)[0]
        for min_r2 in (0.0, cg.median_r2(r2)):
            exp = cg.edges_of_band(r2, min_r2)
            got, count, guard_ok = cg.run_edges(eng, laid, window, min_r2, **kw)
            assert count == len(exp) and guard_ok and 0 < count < full, str(sorted(kw))
            cg.assert_edges_equal(got, exp, str(sorted(kw)))
    d = eng.alloc(4096)                                                                   # exactly one of the two arrays
    for ch, po in ((d, None), (None, d)):
        assert eng.L.hpgv_ld_edges_dev(eng.h, d, 16, 4, 0, 2, ch, po, -1, None, 0.5, d, 4, d, None) == hpgv.ERR_INVALID
    eng.free(d)


def test_edge_cap_and_counter(eng):
    width, nv, window = (64, 64), 300, 100
    codes = cg.planted(width, nv)
    laid = lg.lay(codes, width[0])
    r2 = cg.planted_golden(width, nv, window)[0]
    for min_r2 in (0.0, cg.median_r2(r2), HIGH):
        exp = cg.edges_of_band(r2, min_r2)
        true = len(exp)
        assert true >= 2
        members = set(zip(exp["a"].tolist(), exp["b"].tolist(), mg.bits(exp["r2"]).tolist()))
        for cap in (0, true // 2, true):
            got, count, guard_ok = cg.run_edges(eng, laid, window, min_r2, cap=cap, counter_pattern=0xFFFFFFFFFFFFFFF0 + cap % 7)
            assert count == true, "the counter is overwritten and counts every qualifying pair (cap %d)" % cap
            assert guard_ok, "a record was stored past edge_cap = %d" % cap
            assert len(got) == cap
            stored = list(zip(got["a"].tolist(), got["b"].tolist(), mg.bits(got["r2"]).tolist()))
            assert len(set(stored)) == cap and set(stored) <= members
        cg.assert_edges_equal(got, exp, "edge_cap = the true count")


def test_two_launches_give_the_same_list(eng):
    width, nv, window = (301, 412), 300, 64
    laid = lg.lay(cg.planted(width, nv), width[0])
    a = cg.run_edges(eng, laid, window, 0.0)
    b = cg.run_edges(eng, laid, window, 0.0)
    assert a[1] == b[1] > 0
    cg.assert_edges_equal(a[0], b[0])


def test_refusals(eng):
    d = eng.alloc(8192)
    at = lambda k: C.c_void_p(d.value + k)

    def call(window=2, min_r2=0.5, edges=at(1024), cap=4, counter=at(4096), gt=d, pitch=16, nv=4, b0=0):
        return eng.L.hpgv_ld_edges_dev(eng.h, gt, pitch, nv, b0, window, None, None, -1, None, min_r2, edges, cap, counter, None)
    assert call(min_r2=float("nan")) == hpgv.ERR_INVALID
    assert call(edges=at(1024 + 8)) == hpgv.ERR_INVALID                                   # d_edges: 16-byte aligned
    assert call(counter=at(4096 + 4)) == hpgv.ERR_INVALID and call(counter=None) == hpgv.ERR_INVALID
    assert call(edges=None) == hpgv.ERR_INVALID and call(edges=None, cap=0) == hpgv.OK
    assert call(window=0) == hpgv.ERR_UNSUPPORTED and call(window=1025) == hpgv.ERR_UNSUPPORTED and call(window=-3) == hpgv.ERR_UNSUPPORTED
    assert call(pitch=24) == hpgv.ERR_INVALID and call(pitch=0) == hpgv.ERR_INVALID
    assert call(gt=at(8)) == hpgv.ERR_INVALID
    assert call(b0=5) == hpgv.ERR_INVALID and call(nv=-1) == hpgv.ERR_INVALID
    assert call(b0=4) == hpgv.OK and call(gt=None, nv=0) == hpgv.OK                       # empty work
    assert call(min_r2=float("inf")) == hpgv.OK and call(min_r2=-1.0) == hpgv.OK
    eng.sync()
    eng.free(d)


HOST = ((37, 45), 150, 0, True)


def test_host_entry_point():
    c = mg.case(*HOST)
    cohort = c["cond"] != 2
    e = mg.engine(c)
    rng = np.random.default_rng(8)
    chrom = (np.arange(c["nv"]) // 70).astype(np.int32)
    pos = np.cumsum(rng.integers(1, 100, c["nv"])).astype(np.uint32)
    for window in (7, 64):
        for kw in (dict(), dict(chrom=chrom, pos=pos, max_bp=300)):
            r2 = lg.band(c["codes"][:, cohort], window, **kw)[0]
            for min_r2 in (0.0, cg.median_r2(r2)):
                exp = cg.edges_of_band(r2, min_r2)
                assert len(exp) > 4
                got = e.ld_edges(c["codes"], window, min_r2, **kw)                        # (grows and repeats when 4096 is too few)
                cg.assert_edges_equal(got, exp, "hpgv_ld_edges")                          # as returned: sorted by (b, a)
                same, n = e.ld_edges(c["codes"], window, min_r2, edge_cap=len(exp), **kw)
                assert n == len(exp)
                cg.assert_edges_equal(same, exp, "edge_cap = the count")
                # too little room: the true count, and the caller's list past edge_cap untouched
                room = np.full(len(exp) + 4, 7.0, np.dtype([("a", np.int32), ("b", np.int32), ("r2", np.float64)]))
                n = C.c_uint64(0)
                gt = np.ascontiguousarray(c["codes"])
                chp, pop = (hpgv._ptr(kw["chrom"]), hpgv._ptr(kw["pos"])) if kw else (None, None)
                assert e.L.hpgv_ld_edges(e.h, hpgv._ptr(gt), gt.shape[1], c["nv"], window, chp, pop, kw.get("max_bp", -1), min_r2,
                                         hpgv._ptr(room), len(exp) - 1, C.byref(n)) == hpgv.OK
                assert n.value == len(exp) and (room["a"][len(exp) - 1:] == 7).all()
                assert e.L.hpgv_ld_edges(e.h, hpgv._ptr(gt), gt.shape[1], c["nv"], window, chp, pop, kw.get("max_bp", -1), min_r2,
                                         None, 0, C.byref(n)) == hpgv.OK and n.value == len(exp)
    gt, n = np.ascontiguousarray(c["codes"]), C.c_uint64(9)
    room = np.zeros(16, cg.EDGE)
    call = lambda w, ch, po, nv=c["nv"], m=0.5: e.L.hpgv_ld_edges(e.h, hpgv._ptr(gt), gt.shape[1], nv, w, ch, po, -1, m, hpgv._ptr(room), 16, C.byref(n))
    assert call(4, hpgv._ptr(chrom), None) == hpgv.ERR_INVALID and call(4, None, hpgv._ptr(pos)) == hpgv.ERR_INVALID
    assert call(0, None, None) == hpgv.ERR_UNSUPPORTED and call(1025, None, None) == hpgv.ERR_UNSUPPORTED
    assert call(4, None, None, m=float("nan")) == hpgv.ERR_INVALID
    assert call(4, None, None, 0) == hpgv.OK and n.value == 0
    e.close()


def test_state_and_group_refusals():
    c = mg.case(*HOST)
    gt, n = np.ascontiguousarray(c["codes"]), C.c_uint64(0)
    room = np.zeros(16, cg.EDGE)
    args = (hpgv._ptr(gt), gt.shape[1], c["nv"], 4, None, None, -1, 0.5, hpgv._ptr(room), 16, C.byref(n))
    e = hpgv.Engine(0)                                           # no cohort
    assert e.L.hpgv_ld_edges(e.h, *args) == hpgv.ERR_STATE
    e.close()
    g = mg.engine(c, [0, 0])
    assert g.L.hpgv_ld_edges(g.h, *args) == hpgv.ERR_UNSUPPORTED
    # the device call runs on member 0, as the other *_dev calls do
    cohort = c["cond"] != 2
    m = g.member(0)
    nv, ns = c["codes"].shape
    pitch = m.assoc_layout()[2]
    d_raw, d_lay = m.alloc(nv * ns), m.alloc(nv * pitch)
    m.h2d(d_raw, c["codes"])
    m.layout(hpgv.LAYOUT_ASSOC, d_raw, ns, nv, d_lay)
    m.sync()
    laid = m.d2h(d_lay, (nv, pitch), np.uint8)
    m.free(d_raw), m.free(d_lay)
    r2 = lg.band(c["codes"][:, cohort], 9)[0]
    got, count, guard_ok = cg.run_edges(m, laid, 9, cg.median_r2(r2))
    exp = cg.edges_of_band(r2, cg.median_r2(r2))
    assert count == len(exp) > 0 and guard_ok
    cg.assert_edges_equal(got, exp)
    g.close()
