"""The LD band (include/hpgv.h "LD"): k_ld_window's six counts against int64 numpy products with array_equal and r2 against the
header's expression by bit pattern -- over row widths, variant counts and windows on both sides of every tile edge, with context
rows, skipped rows and the chromosome / distance limits -- and the host, text and group entry points against the device call."""
import ctypes as C

import numpy as np
import pytest

import ld_golden as lg
import model_golden as mg
from helpers import hpgv, random_codes

pytestmark = pytest.mark.gpu

LINE_FILTERED = 0x100                                            # HPGV_LINE_FILTERED of include/hpgv.h


@pytest.fixture(scope="module")
def eng():
    e = lg.engine()
    yield e
    e.close()


def _cover():
    """every value of each axis with the extremes of the other two"""
    W, V, D = lg.WIDTHS, lg.VARIANTS, lg.WINDOWS
    ends = lambda a: (a[0], a[-1])
    cases = {(w, v, d) for w in W for v in ends(V) for d in ends(D)}
    cases |= {(w, v, d) for w in ends(W) for v in V for d in ends(D)}
    cases |= {(w, v, d) for w in ends(W) for v in ends(V) for d in D}
    # a window larger than n_variants that is not the largest one, and the tile edges with a pair across two A tiles
    cases |= {(W[1], 17, 63), (W[1], 17, 100), (W[2], 65, 63), (W[2], 65, 64), (W[1], 150, 200), (W[2], 300, 100)}
    return sorted(cases)


@pytest.mark.parametrize("width,nv,window", _cover())
def test_band(eng, width, nv, window):
    exp = lg.golden(width, nv, window)
    got = lg.run_dev(eng, lg.lay(lg.matrix(width, nv), width[0]), window)
    lg.assert_same(got, exp)
    # without the counts the same r2
    if nv == 300:
        r2, none = lg.run_dev(eng, lg.lay(lg.matrix(width, nv), width[0]), window, counts=False)
        assert none is None and np.array_equal(mg.bits(r2), mg.bits(got[0]))


@pytest.mark.parametrize("window", [10, 100])
def test_b_begin_and_pieces(eng, window):
    width, nv = (37, 45), 300
    codes = lg.matrix(width, nv)
    laid = lg.lay(codes, width[0])
    full = lg.golden(width, nv, window)
    lg.assert_same(lg.run_dev(eng, laid, window, b_begin=37), lg.band(codes, window, b_begin=37))
    r2, c6 = lg.run_dev(eng, laid, window, b_begin=nv)           # nothing to write
    assert r2.shape == (0, window) and c6.shape == (0, window, 6)
    # the matrix cut at 64 and 150: every piece with `window` context rows in front (fewer where the matrix begins)
    skip = np.zeros(nv, np.uint8)
    skip[[63, 64, 149, 170]] = 1
    for sk in (None, skip):
        parts = []
        for lo, hi in ((0, 64), (64, 150), (150, nv)):
            ctx = max(0, lo - window)
            parts.append(lg.run_dev(eng, laid[ctx:hi], window, b_begin=lo - ctx, skip=None if sk is None else sk[ctx:hi]))
        got = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        one = lg.run_dev(eng, laid, window, skip=sk)
        lg.assert_same(one, full if sk is None else lg.band(codes, window, skip=sk))
        assert np.array_equal(got[1], one[1]) and np.array_equal(np.isnan(got[0]), np.isnan(one[0]))
        ok = ~np.isnan(one[0])
        assert np.array_equal(mg.bits(got[0])[ok], mg.bits(one[0])[ok])


def test_special_rows_at_tile_edges(eng):
    width, nv = (301, 412), 150
    codes = lg.matrix(width, nv).copy()
    rng = np.random.default_rng(5)
    codes[16] = 0xFF                                             # all missing: the first row of a wave
    codes[63], codes[64] = 0x00, 0x11                            # monomorphic, on both sides of the A tile edge
    codes[48] = codes[47]                                        # a copy of its neighbour
    codes[80] = lg.flip(codes[79])                               # its neighbour with g -> 2 - g
    codes[31, :256] = np.arange(256)                             # every byte value: half-missing nibbles, 1/2, alleles up to 14
    called = mg.classes(codes[95])[0]
    codes[96] = np.where(called, 0xFF, random_codes(rng, 1, codes.shape[1], quirks=False, p_missing=0.0)[0])
    codes[95, ::7] = 0xFF                                        # (so that row 96 has called samples)
    codes[96, ::7] = 0x01
    codes[96, 7::14] = 0x11
    laid = lg.lay(codes, width[0])
    for window in (10, 64):
        exp = lg.band(codes, window)
        got = lg.run_dev(eng, laid, window)
        lg.assert_same(got, exp)
        r2, c6 = got
        assert np.isnan(r2[16]).all() and not c6[16, :, 0].any() and np.isnan(r2[17:27, :][np.arange(10), np.arange(10)]).all()
        assert np.isnan(r2[63][:10]).all() and np.isnan(r2[64][:10]).all() and c6[64, 0, 0] > 0
        assert r2[48, 0] == 1.0 and r2[80, 0] == 1.0
        n, sa, sb, saa, sbb, sab = c6[80, 0].astype(np.int64)
        assert n * sab - sa * sb < 0
        assert c6[96, 0, 0] == 0 and np.isnan(r2[96, 0]) and c6[96, 1, 0] > 0
        assert np.isfinite(r2[31, :10]).all() and np.isfinite(r2[32:42, :][np.arange(10), np.arange(10)]).all()


def test_skip_chromosomes_and_distances(eng):
    width, nv, window = (37, 45), 150, 20
    codes = lg.matrix(width, nv)
    laid = lg.lay(codes, width[0])
    rng = np.random.default_rng(6)
    skip = (rng.random(nv) < 0.1).astype(np.uint8)
    skip[[15, 16, 64]] = 1
    chrom = np.where(np.arange(nv) < 40, 1, np.where(np.arange(nv) < 128, 2, 7)).astype(np.int32)     # a change inside a tile, one at its edge
    pos = np.cumsum(rng.integers(0, 4, nv) * 50).astype(np.uint32) + 1000                          # steps of 0 (duplicates), 50, 100, 150
    for kw in (dict(skip=skip), dict(chrom=chrom, pos=pos), dict(chrom=chrom, pos=pos, max_bp=500), dict(chrom=chrom, pos=pos, max_bp=499),
               dict(chrom=chrom, pos=pos, max_bp=0), dict(chrom=chrom, pos=pos, max_bp=350, skip=skip),
               dict(chrom=np.zeros(nv, np.int32), pos=pos[::-1].copy(), max_bp=200)):
        exp = lg.band(codes, window, **kw)
        lg.assert_same(lg.run_dev(eng, laid, window, **kw), exp, str(sorted(kw)))
        if kw.get("max_bp") == 500:
            # distances just at the limit are inside, the next step is outside
            dist = np.array([[abs(int(pos[b]) - int(pos[b - d])) if b >= d else -1 for d in range(1, window + 1)] for b in range(nv)])
            assert (dist == 500).any() and (dist == 550).any()
            same = np.array([[b >= d and chrom[b] == chrom[b - d] for d in range(1, window + 1)] for b in range(nv)])
            assert exp[2][(dist == 500) & same].all() and not exp[2][dist == 550].any()
        if kw.get("max_bp") == 0:
            assert exp[2].any() and exp[2].sum() < exp[2].size // 10      # only the duplicate positions
    # exactly one of the two arrays
    d = eng.alloc(4096)
    for ch, po in ((d, None), (None, d)):
        assert eng.L.hpgv_ld_window_dev(eng.h, d, 16, 4, 0, 2, ch, po, -1, None, d, None, None) == hpgv.ERR_INVALID
    eng.free(d)


def test_refusals(eng):
    d = eng.alloc(4096)
    call = lambda gt, pitch, nv, b0, w, r2=C.c_void_p(d.value + 1024): eng.L.hpgv_ld_window_dev(eng.h, gt, pitch, nv, b0, w, None, None, -1, None, r2, None, None)
    assert call(d, 16, 4, 0, 0) == hpgv.ERR_UNSUPPORTED and call(d, 16, 4, 0, 1025) == hpgv.ERR_UNSUPPORTED
    assert call(d, 16, 4, 0, -3) == hpgv.ERR_UNSUPPORTED
    assert call(d, 24, 4, 0, 2) == hpgv.ERR_INVALID and call(d, 0, 4, 0, 2) == hpgv.ERR_INVALID           # pitch
    assert call(C.c_void_p(d.value + 8), 16, 4, 0, 2) == hpgv.ERR_INVALID                                  # d_gt
    assert call(d, 16, 4, 0, 2, C.c_void_p(d.value + 4)) == hpgv.ERR_INVALID                               # d_r2
    assert call(d, 16, 4, 5, 2) == hpgv.ERR_INVALID and call(d, 16, -1, 0, 2) == hpgv.ERR_INVALID          # b_begin, n_variants
    assert call(d, 16, 4, 4, 2) == hpgv.OK and call(None, 16, 0, 0, 2, None) == hpgv.OK                    # empty work
    assert call(d, 16, 4, 0, 2) == hpgv.OK
    eng.sync()
    eng.free(d)


HOST = ((37, 45), 150, 0, True)


def _host_case():
    c = mg.case(*HOST)
    cohort = c["cond"] != 2
    # the golden over the cohort columns; the device call on the engine's own layout of the same rows
    return c, cohort


def _dev_band(e, c, window, **kw):
    nv, ns = c["codes"].shape
    pitch = e.assoc_layout()[2]
    d_raw, d_lay = e.alloc(nv * ns), e.alloc(nv * pitch)
    e.h2d(d_raw, c["codes"])
    e.layout(hpgv.LAYOUT_ASSOC, d_raw, ns, nv, d_lay)
    e.sync()
    laid = e.d2h(d_lay, (nv, pitch), np.uint8)
    e.free(d_raw), e.free(d_lay)
    return lg.run_dev(e, laid, window, **kw)


def test_host_and_text_entry_points():
    c, cohort = _host_case()
    e = mg.engine(c)
    rng = np.random.default_rng(8)
    chrom = (np.arange(c["nv"]) // 70).astype(np.int32)
    pos = np.cumsum(rng.integers(1, 100, c["nv"])).astype(np.uint32)
    for window in (7, 64):
        exp = lg.band(c["codes"][:, cohort], window)
        dev = _dev_band(e, c, window)
        lg.assert_same(dev, exp, "device call on the engine's layout")
        res = e.ld(c["codes"], window)
        lg.assert_same((res["r2"], res["counts6"]), exp, "hpgv_ld")
        assert np.array_equal(np.isnan(res["r2"]), np.isnan(dev[0]))
        only = e.ld(c["codes"], window, counts=False)
        assert only["counts6"] is None and np.array_equal(np.isnan(only["r2"]), np.isnan(res["r2"]))
        res = e.ld(c["codes"], window, chrom=chrom, pos=pos, max_bp=300)
        lg.assert_same((res["r2"], res["counts6"]), lg.band(c["codes"][:, cohort], window, chrom=chrom, pos=pos, max_bp=300), "hpgv_ld, limits")
        rt = e.ld_text(mg.text_of(c["codes"]), window)
        assert rt["n_lines"] == c["nv"] and not rt["status"].any()
        lg.assert_same((rt["r2"], rt["counts6"]), exp, "hpgv_ld_text")
    # exactly one of chrom / pos; window limits; no rows
    gt, r2 = np.ascontiguousarray(c["codes"]), np.zeros((c["nv"], 4))
    call = lambda w, ch, po, nv=c["nv"]: e.L.hpgv_ld(e.h, hpgv._ptr(gt), gt.shape[1], nv, w, ch, po, -1, hpgv._ptr(r2), None)
    assert call(4, hpgv._ptr(chrom), None) == hpgv.ERR_INVALID and call(4, None, hpgv._ptr(pos)) == hpgv.ERR_INVALID
    assert call(0, None, None) == hpgv.ERR_UNSUPPORTED and call(1025, None, None) == hpgv.ERR_UNSUPPORTED
    assert call(4, None, None, 0) == hpgv.OK
    e.close()


def test_text_lines_that_are_skipped_keep_their_slot():
    c, cohort = _host_case()
    e = mg.engine(c)
    codes = c["codes"].copy()
    codes[70] = 0x00
    codes[70, np.flatnonzero(cohort)[3]] = 0x01                  # one alternate allele in the whole row: below the frequency filter
    lines = mg.text_of(codes).split(b"\n")[:-1]
    cut = [0, 40, 149]
    text = b"".join((b"7\t5\trs" if i in cut else l) + b"\n" for i, l in enumerate(lines))      # three lines cut short
    assert e.L.hpgv_set_stats_cohort(e.h, c["ns"]) == hpgv.OK
    assert e.L.hpgv_set_text_filters(e.h, C.c_double(0.02), C.c_double(-1.0), C.c_long(-1)) == hpgv.OK
    window = 12
    rt = e.ld_text(text, window)
    e.close()
    assert rt["n_lines"] == c["nv"]
    assert np.array_equal((rt["status"] & 0xFF) == 1, np.isin(np.arange(c["nv"]), cut))
    # the filter takes row 70, the case's own all-missing and monomorphic rows 1 and 2, and the lines cut short; nothing else
    filtered = (rt["status"] & LINE_FILTERED) != 0
    assert filtered[70] and set(np.flatnonzero(filtered).tolist()) <= {1, 2, 70} | set(cut)
    skip = (filtered | np.isin(np.arange(c["nv"]), cut)).astype(np.uint8)
    exp = lg.band(codes[:, cohort], window, skip=skip)
    lg.assert_same((rt["r2"], rt["counts6"]), exp)
    assert np.isnan(rt["r2"][70]).all() and not rt["counts6"][70].any() and np.isfinite(rt["r2"][69, :10]).all()


def test_state_and_group_refusals():
    c, _ = _host_case()
    gt, r2 = np.ascontiguousarray(c["codes"]), np.zeros((c["nv"], 4))
    text = mg.text_of(c["codes"][:5])
    nl = C.c_int(0)
    e = hpgv.Engine(0)                                           # no cohort
    assert e.L.hpgv_ld(e.h, hpgv._ptr(gt), gt.shape[1], c["nv"], 4, None, None, -1, hpgv._ptr(r2), None) == hpgv.ERR_STATE
    assert e.L.hpgv_ld_text(e.h, text, len(text), 5, C.byref(nl), None, None, None, 4, hpgv._ptr(r2), None) == hpgv.ERR_STATE
    e.close()
    g = mg.engine(c, [0, 0])
    assert g.L.hpgv_ld(g.h, hpgv._ptr(gt), gt.shape[1], c["nv"], 4, None, None, -1, hpgv._ptr(r2), None) == hpgv.ERR_UNSUPPORTED
    assert g.L.hpgv_ld_text(g.h, text, len(text), 5, C.byref(nl), None, None, None, 4, hpgv._ptr(r2), None) == hpgv.ERR_UNSUPPORTED
    # the device call runs on member 0, as the other *_dev calls do
    exp = lg.band(c["codes"][:, c["cond"] != 2], 9)
    lg.assert_same(_dev_band(g.member(0), c, 9), exp)
    g.close()


def test_model_results_are_unchanged_by_an_ld_call():
    c, _ = _host_case()
    e = mg.engine(c)
    before = e.assoc_model(c["codes"])
    e.ld(c["codes"], 100)
    e.ld_text(mg.text_of(c["codes"]), 3)
    after = e.assoc_model(c["codes"])
    text_after = e.assoc_model_text(mg.text_of(c["codes"]))
    e.close()
    assert np.array_equal(before["counts8"], c["c8"])
    for k in ("counts8", "chisq5", "p5"):
        assert np.array_equal(before[k], after[k], equal_nan=True) and np.array_equal(before[k], text_after[k], equal_nan=True), k
    assert np.array_equal(mg.bits(before["chisq5"]), mg.bits(after["chisq5"])) and np.array_equal(mg.bits(before["p5"]), mg.bits(after["p5"]))
