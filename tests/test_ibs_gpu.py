"""The pairwise IBS counts (include/hpgv.h "IBS"): k_ibs_pairs against int64 numpy indicator products with array_equal -- over column
and row counts on both sides of every tile and k-step edge, with pad and garbage columns, skipped and special rows, pieces and
repeated calls -- the class counts, the selection by PI_HAT, and the host and text entry points against the device call."""
import ctypes as C

import numpy as np
import pytest

import ibs_golden as ig
import model_golden as mg
from helpers import hpgv, random_codes

pytestmark = pytest.mark.gpu

LINE_FILTERED = 0x100                                            # HPGV_LINE_FILTERED of include/hpgv.h


@pytest.fixture(scope="module")
def eng():
    e = ig.engine()
    yield e
    e.close()


def _cover():
    """every value of each axis with the extremes of the other, and the shape whose rows are cut into ranges"""
    ends = lambda a: (a[0], a[-1])
    cases = {(c, r) for c in ig.COLS for r in ends(ig.ROWS)} | {(c, r) for c in ends(ig.COLS) for r in ig.ROWS}
    cases |= {(65, 65), (17, 64), ig.SPLIT}
    return sorted(cases)


@pytest.mark.parametrize("cols,rows", _cover())
def test_counts(eng, cols, rows):
    codes, exp = ig.matrix(rows, cols), ig.golden(rows, cols)
    ig.check_counts(ig.run_dev(eng, ig.lay(codes), cols), exp, "pads 0xFF")
    ig.check_counts(ig.run_dev(eng, ig.lay(codes, fill=None), cols), exp, "garbage past n_cols")
    if cols in (17, 130):
        # a pitch far wider than the columns (n_cols == pitch: the runner's 48 samples, test_genome_runner_gpu)
        ig.check_counts(ig.run_dev(eng, ig.lay(codes, pitch=256, fill=None), cols), exp, "wide pitch")


def test_special_rows(eng):
    cols, rows = 130, 300
    codes = ig.matrix(rows, cols).copy()
    rng = np.random.default_rng(5)
    codes[3, :] = np.arange(cols)                                # every byte value over two rows: half-missing nibbles, 1/2, alleles up to 14
    codes[4, :126] = np.arange(130, 256)
    codes[63] = 0xFF                                             # all missing, monomorphic: on both sides of a k-step edge
    codes[64] = 0x11
    codes[128] = 0x00
    codes[:, 16] = 0xFF                                          # an all-missing column, the first of a wave
    codes[:, 70] = codes[:, 7]                                   # a copy across two tiles
    codes[:, 64] = codes[:, 63]                                  # and across the tile edge
    skip = np.zeros(rows, np.uint8)
    skip[[0, 63, 64, 127, 128, 191, 192, 299]] = 1               # the k-step edges, and the first and last row
    skip[rng.random(rows) < 0.05] = 1
    for sk in (None, skip):
        exp = ig.pair_counts(codes, sk)
        got = ig.run_dev(eng, ig.lay(codes, fill=None), cols, sk)
        ig.check_counts(got, exp, "skip" if sk is not None else "")
        assert not got[16, 17:].any() and not got[:16, 16].any()
        assert got[7, 70, 0] > 0 and got[7, 70, 3] == got[7, 70, 0] and got[63, 64, 3] == got[63, 64, 0]
    # a row with a single called column adds nothing; every row skipped adds nothing
    assert not ig.run_dev(eng, ig.lay(codes), cols, np.ones(rows, np.uint8))[np.triu_indices(cols, 1)].any()


def test_pieces_and_repeated_calls(eng):
    cols, rows = 130, 300
    codes, exp = ig.matrix(rows, cols), ig.golden(rows, cols)
    laid = ig.lay(codes)
    skip = np.zeros(rows, np.uint8)
    skip[[63, 64, 149, 170]] = 1
    for sk in (None, skip):
        one = ig.run_dev(eng, laid, cols, sk)
        ig.check_counts(one, exp if sk is None else ig.pair_counts(codes, sk))
        dc = ig.DevCounts(eng, cols)
        for lo, hi in ((0, 64), (64, 150), (150, rows)):
            ig.add_dev(eng, dc, laid[lo:hi], cols, None if sk is None else sk[lo:hi])
        assert np.array_equal(dc.get(), one)
        dc.close()
    dc = ig.DevCounts(eng, cols)
    ig.add_dev(eng, dc, laid, cols)
    ig.add_dev(eng, dc, laid, cols)
    ig.check_counts(dc.get(), 2 * exp, "two calls")
    dc.close()


def test_the_row_ranges_add_up(eng):
    """20 columns are one tile pair: the 5 000 rows are cut into ranges that meet in the atomics"""
    cols, rows = ig.SPLIT
    codes = ig.matrix(rows, cols)
    skip = (np.random.default_rng(2).random(rows) < 0.2).astype(np.uint8)
    ig.check_counts(ig.run_dev(eng, ig.lay(codes, fill=None), cols, skip), ig.pair_counts(codes, skip))


@pytest.mark.parametrize("cols,rows", [(1, 15), (17, 300), (64, 65), (130, 300), (1030, 7)])
def test_class_counts(eng, cols, rows):
    codes = ig.matrix(rows, cols)
    skip = np.zeros(rows, np.uint8)
    skip[::5] = 1
    for sk in (None, skip):
        for fill in (0xFF, None):
            assert np.array_equal(ig.class_dev(eng, ig.lay(codes, fill=fill), cols, sk), ig.class_counts(codes, sk))
    # fewer columns than the matrix holds: the rest is not counted
    if cols > 17:
        assert np.array_equal(ig.class_dev(eng, ig.lay(codes), cols - 5), ig.class_counts(codes[:, :cols - 5]))


@pytest.fixture(scope="module")
def related():
    """130 columns x 300 rows with a duplicate, a parent-child-like pair (one allele shared at every row), an all-missing column"""
    rng = np.random.default_rng(31)
    codes = random_codes(rng, 300, 130, quirks=False, strict=False, p_missing=0.03)
    codes[:, 100] = codes[:, 3]
    codes[rng.random(300) < 0.1, 100] = 0xFF
    hi = codes[:, 8] >> 4
    other = rng.integers(0, 2, 300).astype(np.uint8)
    codes[:, 90] = np.where(codes[:, 8] == 0xFF, 0xFF, (np.minimum(hi, 1) << 4) | other)
    codes[:, 129] = 0xFF
    counts = ig.pair_counts(codes).astype(np.int32)
    E, m = ig.expected(ig.class_counts(codes))
    assert m > 250
    pi = ig.genome_all(counts, E)[..., 3]
    return codes, counts, E, pi


def test_select(eng, related):
    _, counts, E, pi = related
    nc = counts.shape[0]
    d_counts = eng.alloc(counts.nbytes)
    eng.h2d(d_counts, counts)
    gen = hpgv.ibs_genome(counts, E)
    all_pairs = ig.selected(pi, -np.inf)
    assert len(all_pairs) == nc * (nc - 1) // 2 - (nc - 1)       # every pair but the all-missing column's
    for thr in (-1.0, 0.0, 0.05, 0.4, 1.0, 1.5):
        exp = ig.selected(pi, thr)
        got = eng.ibs_select(d_counts, nc, E, thr)
        assert [(int(p["i"]), int(p["j"])) for p in got] == [(i, j) for i, j, _ in exp], thr
        for p in got:
            i, j = int(p["i"]), int(p["j"])
            assert np.array_equal(np.array(p["c"].tolist(), np.int32), counts[i, j])
            assert mg.bits(p["pi_hat"]) == mg.bits(gen[i, j, 3])
        ig.same_bits(got["pi_hat"], [x for _, _, x in exp], "pi_hat against the golden")
    assert (3, 100) in [(i, j) for i, j, _ in ig.selected(pi, 1.0)] and (8, 90) in [(i, j) for i, j, _ in ig.selected(pi, 0.4)]
    assert len(ig.selected(pi, 1.5)) == 0 and 2 < len(ig.selected(pi, 0.05)) < len(all_pairs)
    # a count-only call, and a list shorter than the count: the true count, nothing past the list
    n_all = len(ig.selected(pi, 0.0))
    none, n = eng.ibs_select(d_counts, nc, E, 0.0, cap=0)
    assert none is None and n == n_all
    cap = 37
    assert cap < n_all
    d_pairs, d_n = eng.alloc((cap + 8) * 32), eng.alloc(16)
    eng.h2d(d_pairs, np.full((cap + 8) * 8, ig.PATTERN, np.int32))
    eng.ibs_select_dev(d_counts, nc, E, 0.0, d_pairs, cap, d_n)
    eng.sync()
    assert int(eng.d2h(d_n, (1,), np.uint64)[0]) == n_all
    raw = eng.d2h(d_pairs, (cap + 8,), hpgv.IBS_PAIR)
    assert (raw[cap:].view(np.int32) == ig.PATTERN).all()
    members = {(i, j): x for i, j, x in ig.selected(pi, 0.0)}
    seen = {(int(p["i"]), int(p["j"])) for p in raw[:cap]}
    assert len(seen) == cap and all(k in members for k in seen)
    # one column, none: no pair
    for k in (0, 1):
        pairs, n = eng.ibs_select(d_counts, k, E, -1.0, cap=4)
        assert n == 0 and len(pairs) == 0
    for b in (d_pairs, d_n, d_counts):
        eng.free(b)


def _zeroed(e, ns):
    d = e.alloc(max(ns * ns * 16, 16))
    e.memset_dev(d, 0, ns * ns * 16)
    return d


def test_host_and_text_entry_points(related):
    codes = related[0]
    nv, ns = codes.shape
    e = hpgv.Engine(0)
    pitch = e.set_stats_cohort(ns)
    assert pitch >= ns
    skip = np.zeros(nv, np.uint8)
    skip[[0, 64, 77]] = 1
    for sk in (None, skip):
        exp, exp4 = ig.pair_counts(codes, sk), ig.class_counts(codes, sk)
        d = _zeroed(e, ns)
        c4 = e.ibs(codes, d, skip=sk)
        e.sync()
        got = e.d2h(d, (ns, ns, 4), np.int32)
        assert np.array_equal(c4, exp4) and np.array_equal(got, exp)
        # the device call on the same rows in the engine's own pitch
        dev = ig.run_dev(e, ig.lay(codes, pitch=pitch), ns, sk)
        assert np.array_equal(dev[np.triu_indices(ns, 1)], got[np.triu_indices(ns, 1)])
        # a second batch accumulates
        e.ibs(codes[:100], d)
        e.sync()
        assert np.array_equal(e.d2h(d, (ns, ns, 4), np.int32), exp + ig.pair_counts(codes[:100]))
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
    rt = e.ibs_text(text, d)
    e.sync()
    got = e.d2h(d, (ns, ns, 4), np.int32)
    assert rt["n_lines"] == nv
    assert np.array_equal((rt["status"] & 0xFF) == 1, np.isin(np.arange(nv), cut))
    filtered = (rt["status"] & LINE_FILTERED) != 0
    assert filtered[70] and not filtered[[0, 63, 64, 150]].any()
    tskip = (filtered | np.isin(np.arange(nv), cut + on_x)).astype(np.uint8)
    assert np.array_equal(got, ig.pair_counts(tcodes, tskip)) and np.array_equal(rt["class4"], ig.class_counts(tcodes, tskip))
    assert not rt["class4"][[0, 40, 63, 70]].any() and rt["class4"][1].any()
    dev = ig.run_dev(e, ig.lay(tcodes, pitch=pitch), ns, tskip)
    assert np.array_equal(dev[np.triu_indices(ns, 1)], got[np.triu_indices(ns, 1)])
    # without a status array of the caller's the same
    e.memset_dev(d, 0, ns * ns * 16)
    nl = C.c_int(0)
    c4 = np.zeros((nv, 4), np.int32)
    assert e.L.hpgv_ibs_text(e.h, text, len(text), nv, C.byref(nl), None, None, None, hpgv._ptr(c4), d) == hpgv.OK
    e.sync()
    assert nl.value == nv and np.array_equal(e.d2h(d, (ns, ns, 4), np.int32), got) and np.array_equal(c4, rt["class4"])
    e.free(d)
    e.close()


def test_refusals(eng):
    d = eng.alloc(1 << 16)
    at = lambda off: C.c_void_p(d.value + off)
    pairs = lambda gt, pitch, nv, nc, cnt=at(4096): eng.L.hpgv_ibs_pairs_dev(eng.h, gt, pitch, nv, nc, None, cnt, None)
    cls = lambda gt, pitch, nv, nc, c4=at(4096): eng.L.hpgv_ibs_class_counts_dev(eng.h, gt, pitch, nv, nc, None, c4, None)
    for call in (pairs, cls):
        assert call(d, 24, 4, 8) == hpgv.ERR_INVALID and call(d, 0, 4, 0) == hpgv.ERR_INVALID              # pitch
        assert call(d, 16, 4, 17) == hpgv.ERR_INVALID and call(d, 16, 4, -1) == hpgv.ERR_INVALID            # n_cols
        assert call(d, 16, -1, 8) == hpgv.ERR_INVALID                                                       # n_variants
        assert call(at(8), 16, 4, 8) == hpgv.ERR_INVALID and call(d, 16, 4, 8, at(4096 + 8)) == hpgv.ERR_INVALID
        assert call(None, 16, 0, 8, None) == hpgv.OK                                                        # no rows
    eng.h2d(d, np.full(1 << 14, ig.PATTERN, np.int32))
    assert pairs(d, 16, 4, 1) == hpgv.OK and pairs(d, 16, 4, 0) == hpgv.OK                                  # no pair
    eng.sync()
    assert (eng.d2h(d, (1 << 14,), np.int32) == ig.PATTERN).all()
    E = np.full(5, 0.3)
    sel = lambda cnt, nc, thr, prs, cap, n, Ep=hpgv._ptr(E): eng.L.hpgv_ibs_select_dev(eng.h, cnt, nc, Ep, C.c_double(thr), prs, cap, n, None)
    assert sel(d, 4, float("nan"), at(4096), 4, at(8192)) == hpgv.ERR_INVALID
    assert sel(d, -1, 0.0, at(4096), 4, at(8192)) == hpgv.ERR_INVALID and sel(d, 4, 0.0, None, 4, at(8192)) == hpgv.ERR_INVALID
    assert sel(d, 4, 0.0, at(4096), 4, None) == hpgv.ERR_INVALID and sel(d, 4, 0.0, at(4096), 4, at(8192), None) == hpgv.ERR_INVALID
    assert sel(at(8), 4, 0.0, at(4096), 4, at(8192)) == hpgv.ERR_INVALID and sel(d, 4, 0.0, at(4096 + 8), 4, at(8192)) == hpgv.ERR_INVALID
    assert sel(d, 4, 0.0, at(4096), 4, at(8192 + 4)) == hpgv.ERR_INVALID
    assert sel(d, 4, 0.0, None, 0, at(8192)) == hpgv.OK
    eng.sync()
    # more tile pairs, or more blocks of the counts matrix, than a grid holds: refused before anything is launched
    assert pairs(d, 1 << 23, 4, 1 << 23) == hpgv.ERR_UNSUPPORTED and sel(d, 1 << 20, 0.0, None, 0, at(8192)) == hpgv.ERR_UNSUPPORTED
    eng.free(d)


def test_state_and_group_refusals(related):
    codes = np.ascontiguousarray(related[0][:5])
    ns = codes.shape[1]
    text = mg.text_of(codes)
    nl = C.c_int(0)
    c4 = np.zeros((5, 4), np.int32)
    e = hpgv.Engine(0)                                           # no stats cohort
    d = _zeroed(e, ns)
    assert e.L.hpgv_ibs(e.h, hpgv._ptr(codes), ns, 5, None, hpgv._ptr(c4), d) == hpgv.ERR_STATE
    assert e.L.hpgv_ibs_text(e.h, text, len(text), 5, C.byref(nl), None, None, None, hpgv._ptr(c4), d) == hpgv.ERR_STATE
    e.set_stats_cohort(ns)
    assert e.L.hpgv_ibs(e.h, hpgv._ptr(codes), ns - 1, 5, None, hpgv._ptr(c4), d) == hpgv.ERR_INVALID       # pitch < n_samples
    assert e.L.hpgv_ibs(e.h, hpgv._ptr(codes), ns, 5, None, hpgv._ptr(c4), C.c_void_p(d.value + 8)) == hpgv.ERR_INVALID
    assert e.L.hpgv_ibs(e.h, hpgv._ptr(codes), ns, 5, None, None, d) == hpgv.ERR_INVALID
    assert e.L.hpgv_ibs(e.h, None, ns, 0, None, None, d) == hpgv.OK
    e.free(d)
    e.close()
    g = hpgv.Engine([0, 0])
    assert g.L.hpgv_set_stats_cohort(g.h, ns) == hpgv.OK
    m = g.member(0)
    d = _zeroed(m, ns)
    assert g.L.hpgv_ibs(g.h, hpgv._ptr(codes), ns, 5, None, hpgv._ptr(c4), d) == hpgv.ERR_UNSUPPORTED
    assert g.L.hpgv_ibs_text(g.h, text, len(text), 5, C.byref(nl), None, None, None, hpgv._ptr(c4), d) == hpgv.ERR_UNSUPPORTED
    # the device call runs on member 0, as the other *_dev calls do
    dev = ig.run_dev(m, ig.lay(codes), ns)
    ig.check_counts(dev, ig.pair_counts(codes))
    m.free(d)
    g.close()
