"""The genetic relationship matrix on the device (include/hpgv.h "GRM"): k_grm_pairs's {sq, n} against int64 numpy products with
array_equal -- over column and row counts on both sides of every tile and k-step edge and past the row-range cap, with pad and
garbage columns, at frac_bits 11 and at 14 with min_maf 0.5, with skipped and special rows, pieces and repeated calls --,
k_grm_table against the host function, and the host and text entry points against the device calls."""
import ctypes as C

import numpy as np
import pytest

import grm_golden as gg
import ibs_golden as ig
import model_golden as mg
from helpers import hpgv, random_codes

pytestmark = pytest.mark.gpu

LINE_FILTERED = 0x100                                            # HPGV_LINE_FILTERED of include/hpgv.h
CAPPED = (20, 70000)                                             # columns x rows: past GRM_MAX_RANGE_ROWS and past 66 052 rows


@pytest.fixture(scope="module")
def eng():
    e = ig.engine()
    yield e
    e.close()


def _cover():
    """every value of each axis with the extremes of the other, the shape whose rows are cut into ranges, the one past the cap"""
    ends = lambda a: (a[0], a[-1])
    cases = {(c, r) for c in ig.COLS for r in ends(ig.ROWS)} | {(c, r) for c in ends(ig.COLS) for r in ig.ROWS}
    cases |= {(65, 65), (17, 64), ig.SPLIT, CAPPED}
    return sorted(cases)


def _matrix(rows, cols, which):
    return ig.matrix(rows, cols) if which == 0 else gg.balanced(rows, cols)


@pytest.mark.parametrize("which", [0, 1], ids=["s11", "s14"])
@pytest.mark.parametrize("cols,rows", _cover())
def test_sums(eng, cols, rows, which):
    codes, G, (s, maf) = _matrix(rows, cols, which), gg.golden_of(rows, cols, which), (gg.DEFAULT, gg.EXTREME)[which]
    if rows >= 64:
        assert G["used"].sum() >= rows // 4 and (which == 0 or (~G["used"]).any())
    gg.check_acc(gg.run_dev(eng, ig.lay(codes), cols, s, maf), G["acc"], "pads 0xFF")
    gg.check_acc(gg.run_dev(eng, ig.lay(codes, fill=None), cols, s, maf), G["acc"], "garbage past n_cols")
    if cols in (17, 130):
        gg.check_acc(gg.run_dev(eng, ig.lay(codes, pitch=256, fill=None), cols, s, maf), G["acc"], "wide pitch")


def test_the_capped_shape_is_cut_into_ranges(eng):
    """what test_sums's CAPPED case runs: more rows than one i32 sum may hold, which only ranges that meet in the int64 atomics
    carry.  (With 20 columns the ranges are short because the tile pairs are few; the cap's own path needs about a thousand tile
    pairs and is checked on the plan, tests/test_grm_cpu.py.)"""
    cols, rows = CAPPED
    per = hpgv.grm_plan_rows(rows, cols, 256)
    assert rows > 66052 and per <= 32768 and rows // per >= 2


def test_table_kernel_is_the_host_function(eng):
    cols, rows = 130, 300
    skip = np.zeros(rows, np.uint8)
    skip[[0, 63, 64, 255, 256, 299]] = 1
    for which in (0, 1):
        codes, (s, maf) = _matrix(rows, cols, which), (gg.DEFAULT, gg.EXTREME)[which]
        for sk in (None, skip):
            c4 = ig.class_counts(codes, sk)
            used, tab = hpgv.grm_table(c4, s, maf)
            if sk is not None:
                used = used & (sk == 0)
                tab[~used] = 0
            da = gg.DevAcc(eng, cols)
            d_tab, d_skip, n_used = gg.add_dev(eng, da, ig.lay(codes), cols, s, maf, sk)
            da.close()
            assert np.array_equal(d_tab["hi"], tab["hi"]) and np.array_equal(d_tab["lo"], tab["lo"])
            assert np.array_equal(d_skip != 0, ~used) and n_used == int(used.sum()) and 0 < n_used and (n_used < rows or (which == 0 and sk is None))
            if sk is not None:
                assert (d_skip[sk != 0] == 1).all()


def test_special_rows(eng):
    cols, rows = 130, 300
    codes = ig.matrix(rows, cols).copy()
    rng = np.random.default_rng(5)
    codes[3, :] = np.arange(cols)                                # every byte value over two rows: half-missing nibbles, 1/2, alleles up to 14
    codes[4, :126] = np.arange(130, 256)
    codes[63] = 0xFF                                             # all missing, monomorphic: on both sides of a k-step edge
    codes[64] = 0x11
    codes[128] = 0x00
    codes[127] = 0x00                                            # three alternate alleles among 260: MAF just above 0.01, the largest |q| in use
    codes[127, [5, 77]] = (0x11, 0x01)
    codes[191] = 0x00                                            # two: MAF below 0.01, unused
    codes[191, [6, 78]] = (0x01, 0x10)
    codes[:, 16] = 0xFF                                          # an all-missing column, the first of a wave
    codes[:, 70] = codes[:, 7]                                   # a copy across two tiles
    codes[:, 64] = codes[:, 63]                                  # and across the tile edge
    skip = np.zeros(rows, np.uint8)
    skip[[0, 63, 64, 128, 192, 299]] = 1                         # the k-step edges, and the first and last row
    skip[rng.random(rows) < 0.05] = 1
    skip[127] = 0
    s, maf = gg.DEFAULT
    for sk in (None, skip):
        G = gg.golden(codes, s, maf, sk)
        assert G["used"][127] and not G["used"][[63, 191]].any() and np.abs(G["q"][127]).max() > 100 * 256
        if sk is None:
            assert not G["used"][[64, 128]].any()
        got = gg.run_dev(eng, ig.lay(codes, fill=None), cols, s, maf, sk)
        gg.check_acc(got, G["acc"], "skip" if sk is not None else "")
        # the all-missing column: nothing, not even its diagonal; the copies: the diagonal's sums
        assert not got[16, 16:].any() and not got[:17, 16].any()
        assert got[7, 7, 1] > 0 and np.array_equal(got[7, 70], got[7, 7]) and np.array_equal(got[70, 70], got[7, 7]) and np.array_equal(got[63, 64], got[63, 63])
        # the diagonal is written, and is a sum of squares
        d = np.arange(cols)
        assert (got[d, d, 1][np.arange(cols) != 16] > 0).all() and (got[d, d, 0] >= 0).all()
    iu = np.triu_indices(cols)
    assert not gg.run_dev(eng, ig.lay(codes), cols, s, maf, np.ones(rows, np.uint8))[iu].any()


def test_pieces_and_repeated_calls(eng):
    cols, rows = 130, 300
    s, maf = gg.DEFAULT
    codes, exp = ig.matrix(rows, cols), gg.golden_of(rows, cols, 0)["acc"]
    laid = ig.lay(codes)
    skip = np.zeros(rows, np.uint8)
    skip[[63, 64, 149, 170]] = 1
    for sk in (None, skip):
        one = gg.run_dev(eng, laid, cols, s, maf, sk)
        gg.check_acc(one, exp if sk is None else gg.golden(codes, s, maf, sk)["acc"])
        da = gg.DevAcc(eng, cols)
        for lo, hi in ((0, 64), (64, 150), (150, rows)):
            gg.add_dev(eng, da, laid[lo:hi], cols, s, maf, None if sk is None else sk[lo:hi])
        assert np.array_equal(da.get(), one)
        da.close()
    da = gg.DevAcc(eng, cols)
    gg.add_dev(eng, da, laid, cols, s, maf)
    gg.add_dev(eng, da, laid, cols, s, maf)
    gg.check_acc(da.get(), 2 * exp, "two calls")
    da.close()


def _zeroed(e, ns):
    d = e.alloc(max(ns * ns * 16, 16))
    e.memset_dev(d, 0, ns * ns * 16)
    return d


@pytest.fixture(scope="module")
def cohort():
    rng = np.random.default_rng(31)
    return random_codes(rng, 300, 130, quirks=False, strict=False, p_missing=0.03)


def test_host_and_text_entry_points(cohort):
    codes = cohort
    nv, ns = codes.shape
    s, maf = gg.DEFAULT
    e = hpgv.Engine(0)
    pitch = e.set_stats_cohort(ns)
    iu = np.triu_indices(ns)
    skip = np.zeros(nv, np.uint8)
    skip[[0, 64, 77]] = 1
    for sk in (None, skip):
        G = gg.golden(codes, s, maf, sk)
        d = _zeroed(e, ns)
        c4 = e.grm(codes, d, s, maf, skip=sk)
        e.sync()
        got = e.d2h(d, (ns, ns, 2), np.int64)
        assert np.array_equal(c4, G["class4"]) and np.array_equal(got, G["acc"])
        # the device calls on the same rows in the engine's own pitch
        dev = gg.run_dev(e, ig.lay(codes, pitch=pitch), ns, s, maf, sk)
        assert np.array_equal(dev[iu], got[iu])
        # a second batch accumulates
        e.grm(codes[:100], d, s, maf)
        e.sync()
        assert np.array_equal(e.d2h(d, (ns, ns, 2), np.int64), G["acc"] + gg.golden(codes[:100], s, maf)["acc"])
        e.free(d)
    # the text form: a line cut short, a line the frequency filter rejects, chromosome-X lines
    tcodes = codes.copy()
    tcodes[70] = 0x00
    tcodes[70, 5] = 0x01                                         # one alternate allele in the whole row: below the frequency filter
    lines = mg.text_of(tcodes).split(b"\n")[:-1]
    cut, on_x = [40, 299], [0, 63, 64, 150]
    text = b"".join((b"7\t5\trs" if i in cut else (b"X" + l[1:] if i in on_x else l)) + b"\n" for i, l in enumerate(lines))
    assert e.L.hpgv_set_text_filters(e.h, C.c_double(0.02), C.c_double(-1.0), C.c_long(-1)) == hpgv.OK
    d = _zeroed(e, ns)
    rt = e.grm_text(text, d, s, maf)
    e.sync()
    got = e.d2h(d, (ns, ns, 2), np.int64)
    assert rt["n_lines"] == nv
    filtered = (rt["status"] & LINE_FILTERED) != 0
    assert filtered[70] and not filtered[[0, 63, 64, 150]].any()
    tskip = (filtered | np.isin(np.arange(nv), cut + on_x)).astype(np.uint8)
    G = gg.golden(tcodes, s, maf, tskip)
    assert np.array_equal(got, G["acc"]) and np.array_equal(rt["class4"], G["class4"])
    assert not rt["class4"][[0, 40, 63, 70]].any() and rt["class4"][1].any() and got[iu][:, 1].all()
    dev = gg.run_dev(e, ig.lay(tcodes, pitch=pitch), ns, s, maf, tskip)
    assert np.array_equal(dev[iu], got[iu])
    # more lines than room: n_lines says so and NOTHING was added
    e.memset_dev(d, 0, ns * ns * 16)
    rt2 = e.grm_text(text, d, s, maf, max_lines=nv - 10)
    e.sync()
    assert rt2["n_lines"] > nv - 10 and not e.d2h(d, (ns, ns, 2), np.int64).any()
    # without a status array of the caller's the same as with one
    nl = C.c_int(0)
    c4 = np.zeros((nv, 4), np.int32)
    assert e.L.hpgv_grm_text(e.h, text, len(text), nv, C.byref(nl), None, None, None, s, C.c_double(maf), hpgv._ptr(c4), d) == hpgv.OK
    e.sync()
    assert nl.value == nv and np.array_equal(e.d2h(d, (ns, ns, 2), np.int64), got) and np.array_equal(c4, rt["class4"])
    e.free(d)
    e.close()


def test_refusals(eng):
    d = eng.alloc(1 << 16)
    at = lambda off: C.c_void_p(d.value + off)
    pairs = lambda gt, pitch, nv, nc, acc=at(4096), tab=at(8192): eng.L.hpgv_grm_pairs_dev(eng.h, gt, pitch, nv, nc, None, tab, acc, None)
    assert pairs(d, 24, 4, 8) == hpgv.ERR_INVALID and pairs(d, 0, 4, 0) == hpgv.ERR_INVALID                 # pitch
    assert pairs(d, 16, 4, 17) == hpgv.ERR_INVALID and pairs(d, 16, 4, -1) == hpgv.ERR_INVALID              # n_cols
    assert pairs(d, 16, -1, 8) == hpgv.ERR_INVALID                                                          # n_variants
    assert pairs(at(8), 16, 4, 8) == hpgv.ERR_INVALID and pairs(d, 16, 4, 8, at(4096 + 8)) == hpgv.ERR_INVALID
    assert pairs(d, 16, 4, 8, at(4096), at(8192 + 4)) == hpgv.ERR_INVALID and pairs(d, 16, 4, 8, at(4096), None) == hpgv.ERR_INVALID
    assert pairs(None, 16, 0, 8, None, None) == hpgv.OK                                                     # no rows
    eng.h2d(d, np.full(1 << 14, 0x5A5A5A5A, np.int32))
    assert pairs(d, 16, 4, 0) == hpgv.OK and pairs(d, 16, 0, 8) == hpgv.OK                                  # no column, no row: nothing written
    eng.sync()
    assert (eng.d2h(d, (1 << 14,), np.int32) == 0x5A5A5A5A).all()
    assert pairs(d, 1 << 23, 4, 1 << 23) == hpgv.ERR_UNSUPPORTED                                            # more tile pairs than a grid holds
    tab = lambda c4, nv, s, maf, skip=at(1024), t=at(8192), n=at(2048): eng.L.hpgv_grm_table_dev(eng.h, c4, nv, s, C.c_double(maf), skip, t, n, None)
    assert tab(d, -1, 11, 0.01) == hpgv.ERR_INVALID
    assert tab(d, 4, -1, 0.01) == hpgv.ERR_INVALID and tab(d, 4, 15, 0.01) == hpgv.ERR_INVALID
    assert tab(d, 4, 11, -0.1) == hpgv.ERR_INVALID and tab(d, 4, 11, 0.51) == hpgv.ERR_INVALID and tab(d, 4, 11, float("nan")) == hpgv.ERR_INVALID
    assert tab(at(8), 4, 11, 0.01) == hpgv.ERR_INVALID and tab(d, 4, 11, 0.01, at(1024), at(8192 + 4)) == hpgv.ERR_INVALID
    assert tab(d, 4, 11, 0.01, at(1024), at(8192), at(2048 + 2)) == hpgv.ERR_INVALID
    assert tab(d, 4, 11, 0.01, None) == hpgv.ERR_INVALID and tab(None, 4, 11, 0.01) == hpgv.ERR_INVALID and tab(d, 4, 11, 0.01, at(1024), None) == hpgv.ERR_INVALID
    assert tab(None, 0, 11, 0.01, None, None) == hpgv.OK                                                    # no rows: the count is zeroed
    eng.sync()
    assert int(eng.d2h(at(2048), (1,), np.int32)[0]) == 0
    assert tab(d, 4, 11, 0.01, at(1024), at(8192), None) == hpgv.OK                                         # the count is optional
    eng.sync()
    eng.free(d)


def test_state_and_group_refusals(cohort):
    codes = np.ascontiguousarray(cohort[:5])
    ns = codes.shape[1]
    text = mg.text_of(codes)
    nl = C.c_int(0)
    c4 = np.zeros((5, 4), np.int32)
    s, maf = 11, C.c_double(0.01)
    e = hpgv.Engine(0)                                           # no stats cohort
    d = _zeroed(e, ns)
    assert e.L.hpgv_grm(e.h, hpgv._ptr(codes), ns, 5, None, s, maf, hpgv._ptr(c4), d) == hpgv.ERR_STATE
    assert e.L.hpgv_grm_text(e.h, text, len(text), 5, C.byref(nl), None, None, None, s, maf, hpgv._ptr(c4), d) == hpgv.ERR_STATE
    e.set_stats_cohort(ns)
    assert e.L.hpgv_grm(e.h, hpgv._ptr(codes), ns - 1, 5, None, s, maf, hpgv._ptr(c4), d) == hpgv.ERR_INVALID      # pitch < n_samples
    assert e.L.hpgv_grm(e.h, hpgv._ptr(codes), ns, 5, None, s, maf, hpgv._ptr(c4), C.c_void_p(d.value + 8)) == hpgv.ERR_INVALID
    assert e.L.hpgv_grm(e.h, hpgv._ptr(codes), ns, 5, None, s, maf, None, d) == hpgv.ERR_INVALID
    assert e.L.hpgv_grm(e.h, hpgv._ptr(codes), ns, 5, None, s, maf, hpgv._ptr(c4), None) == hpgv.ERR_INVALID
    assert e.L.hpgv_grm(e.h, hpgv._ptr(codes), ns, 5, None, 15, maf, hpgv._ptr(c4), d) == hpgv.ERR_INVALID
    assert e.L.hpgv_grm(e.h, hpgv._ptr(codes), ns, 5, None, s, C.c_double(0.7), hpgv._ptr(c4), d) == hpgv.ERR_INVALID
    assert e.L.hpgv_grm_text(e.h, text, len(text), 5, C.byref(nl), None, None, None, -1, maf, hpgv._ptr(c4), d) == hpgv.ERR_INVALID
    assert e.L.hpgv_grm(e.h, None, ns, 0, None, s, maf, None, d) == hpgv.OK
    e.sync()
    assert not e.d2h(d, (ns, ns, 2), np.int64).any()
    e.free(d)
    e.close()
    g = hpgv.Engine([0, 0])
    assert g.L.hpgv_set_stats_cohort(g.h, ns) == hpgv.OK
    m = g.member(0)
    d = _zeroed(m, ns)
    assert g.L.hpgv_grm(g.h, hpgv._ptr(codes), ns, 5, None, s, maf, hpgv._ptr(c4), d) == hpgv.ERR_UNSUPPORTED
    assert g.L.hpgv_grm_text(g.h, text, len(text), 5, C.byref(nl), None, None, None, s, maf, hpgv._ptr(c4), d) == hpgv.ERR_UNSUPPORTED
    # the device calls run on member 0, as the other *_dev calls do
    gg.check_acc(gg.run_dev(m, ig.lay(codes), ns, 11, 0.01), gg.golden(codes, 11, 0.01)["acc"])
    m.free(d)
    g.close()
