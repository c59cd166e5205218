"""Allele scoring on the device (include/hpgv.h "Score"): k_score_cols's int64 sums against numpy products with array_equal -- over
column, row and score counts on both sides of every tile, k-step and score-group edge, with pad and garbage columns, flipped and
skipped rows, with and without imputation --, one-hot matrices that pin which variant of the table meets which row of the matrix,
the limbs at their extremes over more rows than one i32 sum holds, k_score_table against the host function, pieces on two
streams and repeated calls, and the host and text entry points against the device calls."""
import ctypes as C

import numpy as np
import pytest

import ibs_golden as ig
import model_golden as mg
import score_golden as sg
from helpers import hpgv, random_codes

pytestmark = pytest.mark.gpu

LINE_FILTERED = 0x100                                            # HPGV_LINE_FILTERED of include/hpgv.h
COLS = [1, 15, 16, 17, 63, 64, 65, 130, 257]
ROWS = [1, 15, 16, 17, 63, 64, 65, 127, 129, 300]
SCORES = [1, 3, 4, 5, 8, 24, 32]
LONG = (20, (1 << 22) + 192)                                     # columns x rows: past SCORE_MAX_RANGE_ROWS


@pytest.fixture(scope="module")
def eng():
    e = ig.engine()
    yield e
    e.close()


def _cover():
    """every value of each axis with the extremes of the others"""
    ends = lambda a: (a[0], a[-1])
    cases = {(c, r, k) for c in COLS for r in ends(ROWS) for k in ends(SCORES)}
    cases |= {(c, r, k) for c in ends(COLS) for r in ROWS for k in ends(SCORES)}
    cases |= {(c, r, k) for c in ends(COLS) for r in ends(ROWS) for k in SCORES}
    cases |= {(65, 65, 5), (17, 64, 4), (130, 129, 24)}
    return sorted(cases)


@pytest.mark.parametrize("cols,rows,ns", _cover())
def test_sums(eng, cols, rows, ns):
    codes = ig.matrix(rows, cols)
    w, s, flags = sg.random_inputs(rows, ns, 1000 * cols + rows + ns)
    for impute in (1, 0):
        G = sg.golden(codes, w, s, flags, impute)
        if rows >= 64:
            assert G["used"].sum() >= rows // 2 and (flags & sg.FLIP).any() and (flags & sg.SKIP).any()
        sg.check_acc(sg.run_dev(eng, ig.lay(codes), cols, w, s, flags, impute), G, "pads 0xFF, impute %d" % impute)
        sg.check_acc(sg.run_dev(eng, ig.lay(codes, fill=None), cols, w, s, flags, impute), G, "garbage past n_cols, impute %d" % impute)
        if cols in (17, 130):
            sg.check_acc(sg.run_dev(eng, ig.lay(codes, pitch=272, fill=None), cols, w, s, flags, impute), G, "wide pitch, impute %d" % impute)


@pytest.mark.parametrize("ns", [1, 5])
@pytest.mark.parametrize("cols", [1, 16, 23, 130])
def test_one_hot_k_order(eng, cols, ns):
    """all 0x00 but one 0x01 at (row r, column r mod cols), row r weighing q_r = r + 1 at s = 0: sum[col] is the sum of the q_r of
    that column's rows and nothing else -- the variant of the A operand's byte is the row of the B operand's.  Then with the single
    call made missing and imputation on: p = 0, so the missing byte's own term is 0 and nothing at all may arrive."""
    rows = 130
    r = np.arange(rows)
    codes = np.zeros((rows, cols), np.uint8)
    codes[r, r % cols] = 0x01
    w = np.repeat((r + 1.0)[:, None], ns, axis=1) * (np.arange(ns) + 1.0)[None, :]
    s, flags = np.zeros(ns, np.int32), np.zeros(rows, np.uint8)
    exp = np.zeros((ns + 2, cols), np.int64)
    for k in range(ns):
        np.add.at(exp[k], r % cols, (r + 1) * (k + 1))
    exp[ns] = rows
    np.add.at(exp[ns + 1], r % cols, 1)
    G = sg.golden(codes, w, s, flags, 1)
    assert np.array_equal(G["acc"], exp)
    sg.check_acc(sg.run_dev(eng, ig.lay(codes), cols, w, s, flags, 1), G, "one-hot")
    # each row alone: its weight arrives in its column
    for one in (0, 15, 16, 63, 64, 129):
        f1 = np.full(rows, sg.SKIP, np.uint8)
        f1[one] = 0
        acc, _ = sg.run_dev(eng, ig.lay(codes), cols, w, s, f1, 1)
        assert acc[0, one % cols] == one + 1 and np.count_nonzero(acc[0, :cols]) == 1, one
    miss = codes.copy()
    miss[r, r % cols] = 0xFF
    if cols > 1:
        G = sg.golden(miss, w, s, flags, 1)
        assert not G["acc"][:ns].any() and (G["acc"][ns] < rows).all()
        sg.check_acc(sg.run_dev(eng, ig.lay(miss), cols, w, s, flags, 1), G, "one-hot missing")
    # the missing byte's imputed term itself: a second column of 0x11 makes p > 0, each row's q_m distinct
    if cols > 1:
        m2 = miss.copy()
        m2[r, (r + 1) % cols] = 0x11
        G = sg.golden(m2, w * 64.0, s, flags, 1)
        assert len(np.unique(G["qm"][:, 0])) > rows // 2
        sg.check_acc(sg.run_dev(eng, ig.lay(m2), cols, w * 64.0, s, flags, 1), G, "one-hot imputed")


def test_the_long_shape_is_cut_into_ranges(eng):
    cols, rows = LONG
    per = hpgv.score_plan_rows(rows, cols, 1, 256)
    assert rows > 1 << 22 and per <= 1 << 22 and -(-rows // per) >= 2


@pytest.mark.parametrize("low,sign", [(-128, 1), (127, 1), (-128, -1), (127, -1)])
def test_limb_extremes_over_a_long_range(eng, low, sign):
    """weights whose three low limbs are all `low` with the top limb the largest of its sign at which |q| <= 2^28, genotypes all
    2, more rows than the cap: the ranges meet in the int64 atomics"""
    cols, rows = LONG
    base = low * (1 + 256 + 65536)
    top = max(t for t in range(1, 65) if abs(base + sign * t * (1 << 24)) <= 2 ** 28) * sign
    q = base + top * (1 << 24)
    assert abs(top) in (15, 16) and abs(q + sign * (1 << 24)) > 2 ** 28 and np.array_equal(sg.limbs(np.int64(q)), [low, low, low, top])
    laid = np.full((rows, 32), 0x11, np.uint8)
    laid[:, cols:] = 0xFF
    w = np.full((rows, 1), float(q))
    flags = np.zeros(rows, np.uint8)
    acc, const = sg.run_dev(eng, laid, cols, w, [0], flags, 0)
    assert (acc[0, :cols] == 2 * q * rows).all() and (acc[1, :cols] == rows).all() and (acc[2, :cols] == 2 * rows).all()
    assert (acc[:, cols:] == sg.PATTERN).all() and const.tolist() == [0, rows]


def test_table_kernel_is_the_host_function(eng):
    cols, rows, ns = 130, 300, 5
    codes = ig.matrix(rows, cols)
    w, s, flags = sg.random_inputs(rows, ns, 5)
    w[7, 2] = 2.0 ** 40                                          # |q| past 2^28: the row is unused
    skip = np.zeros(rows, np.uint8)
    skip[[0, 63, 64, 255, 256, 299]] = 1
    for impute in (0, 1):
        for sk in (None, skip):
            out = ((flags & sg.SKIP) != 0) | (False if sk is None else sk != 0)
            c4 = ig.class_counts(codes, out.astype(np.uint8))
            used, lim, c = hpgv.score_table(c4, w, s, np.where(out, flags | sg.SKIP, flags), impute)
            assert not used[7] and used.sum() > rows // 2 and not lim[~used].any()
            da = sg.DevAcc(eng, ns, cols)
            d_tab, d_skip = sg.add_dev(eng, da, ig.lay(codes), cols, w, s, flags, impute, sk, tab_pitch=384)
            _, const = da.get()
            da.close()
            exp = np.zeros((ns, 8, 384), np.int8)
            exp[:, :, :rows] = lim.transpose(1, 2, 0)
            assert np.array_equal(d_tab, exp.reshape(ns * 8, 384))
            assert np.array_equal(d_skip != 0, ~used) and (d_skip[out] == 1).all()
            assert np.array_equal(const, np.concatenate([c.sum(axis=0), [used.sum()]]))


def test_special_rows(eng):
    cols, rows, ns = 130, 300, 3
    codes = ig.matrix(rows, cols).copy()
    codes[3, :] = np.arange(cols)                                # every byte value over two rows
    codes[4, :126] = np.arange(130, 256)
    codes[60] = 0xFF                                             # an all-missing row: unused
    codes[61] = 0x00                                             # monomorphic rows: used, they have a score
    codes[62] = 0x11
    codes[:, 16] = 0xFF                                          # an all-missing column, the first of a wave
    w, s, flags0 = sg.random_inputs(rows, ns, 9, p_skip=0.0)
    flags0[[0, 299]] = sg.SKIP | sg.FLIP
    flags0[[60, 61, 62]] = (0, sg.FLIP, 0)
    edges = [63, 64, 128]                                        # the rows at the k-step edges: each skipped, each flipped, each plain
    for edge_flag in (sg.SKIP, sg.FLIP, 0):
        flags = flags0.copy()
        flags[edges] = edge_flag
        for impute in (0, 1):
            G = sg.golden(codes, w, s, flags, impute)
            assert not G["used"][[60, 0, 299]].any() and G["used"][[61, 62]].all() and G["used"][edges].all() == (edge_flag != sg.SKIP)
            got = sg.run_dev(eng, ig.lay(codes, fill=None), cols, w, s, flags, impute)
            sg.check_acc(got, G, "edges %d, impute %d" % (edge_flag, impute))
            acc, const = got
            avg, cnt = sg.average(acc[:, :cols], const, s, impute)
            assert acc[ns, 16] == 0 and acc[ns + 1, 16] == 0
            if impute:
                assert np.isfinite(avg).all() and acc[:ns, 16].any()
            else:
                assert np.isnan(avg[:, 16]).all() and np.isfinite(np.delete(avg, 16, axis=1)).all()
                # without imputation a missing byte gives exactly 0, flipped or not: the flipped rows' -2 q cancel the constant
                assert const[:ns].all() and (sg.value(acc[:, :cols], const, s)[:, 16] == 0.0).all()
    # every row skipped: nothing at all
    acc, const = sg.run_dev(eng, ig.lay(codes), cols, w, s, flags0, 1, np.ones(rows, np.uint8))
    assert not acc[:, :cols].any() and not const.any()


def test_pieces_streams_and_repeated_calls(eng):
    cols, rows, ns = 130, 300, 5
    codes = ig.matrix(rows, cols)
    laid = ig.lay(codes)
    w, s, flags = sg.random_inputs(rows, ns, 21)
    streams = [C.c_void_p(), C.c_void_p()]
    for st in streams:
        assert eng.L.hpgv_stream_create(eng.h, C.byref(st)) == hpgv.OK
    for impute in (0, 1):
        G = sg.golden(codes, w, s, flags, impute)
        one = sg.run_dev(eng, laid, cols, w, s, flags, impute)
        sg.check_acc(one, G)
        # (class counts run over the columns of a row: a piece's rows have the whole matrix's, and the pieces' goldens add up)
        parts = ((0, 64), (64, 150), (150, rows))
        exp = [sg.golden(codes[lo:hi], w[lo:hi], s, flags[lo:hi], impute) for lo, hi in parts]
        da = sg.DevAcc(eng, ns, cols)
        queued = [sg.queue_dev(eng, da, laid[lo:hi], cols, w[lo:hi], s, flags[lo:hi], impute, stream=streams[i & 1]) for i, (lo, hi) in enumerate(parts)]
        for q in queued:
            sg.finish_dev(eng, q)
        got = da.get()
        da.close()
        sg.check_acc(got, dict(acc=sum(x["acc"] for x in exp), const=sum(x["const"] for x in exp)), "three pieces on two streams")
        assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1])       # (rows are independent: the same bytes)
        da = sg.DevAcc(eng, ns, cols)
        sg.add_dev(eng, da, laid, cols, w, s, flags, impute)
        sg.add_dev(eng, da, laid, cols, w, s, flags, impute)
        sg.check_acc(da.get(), dict(acc=2 * G["acc"], const=2 * G["const"]), "two calls")
        da.close()
    for st in streams:
        assert eng.L.hpgv_stream_destroy(eng.h, st) == hpgv.OK


def _zeroed(e, ns, n_scores):
    pitch = sg.acc_pitch_of(ns)
    d, dc = e.alloc((n_scores + 2) * pitch * 8), e.alloc((n_scores + 1) * 8)
    e.memset_dev(d, 0, (n_scores + 2) * pitch * 8)
    e.memset_dev(dc, 0, (n_scores + 1) * 8)
    return d, dc, pitch


def _read(e, d, dc, ns, n_scores):
    e.sync()
    return e.d2h(d, (n_scores + 2, sg.acc_pitch_of(ns)), np.int64)[:, :ns], e.d2h(dc, (n_scores + 1,), np.int64)


@pytest.fixture(scope="module")
def cohort():
    rng = np.random.default_rng(31)
    return random_codes(rng, 300, 130, quirks=False, strict=False, p_missing=0.03)


def test_host_and_text_entry_points(cohort):
    codes = cohort
    nv, ns, k = codes.shape + (3,)
    w, s, flags = sg.random_inputs(nv, k, 41)
    e = hpgv.Engine(0)
    pitch = e.set_stats_cohort(ns)
    for impute in (0, 1):
        G = sg.golden(codes, w, s, flags, impute)
        d, dc, ap = _zeroed(e, ns, k)
        c4 = e.score(codes, w, flags, s, impute, d, ap, dc)
        acc, const = _read(e, d, dc, ns, k)
        assert np.array_equal(c4, G["class4"]) and np.array_equal(acc, G["acc"]) and np.array_equal(const, G["const"])
        # the device calls on the same rows in the engine's own pitch
        sg.check_acc(sg.run_dev(e, ig.lay(codes, pitch=pitch), ns, w, s, flags, impute), G)
        # a second batch accumulates
        e.score(codes[:100], w[:100], flags[:100], s, impute, d, ap, dc)
        G2 = sg.golden(codes[:100], w[:100], s, flags[:100], impute)
        acc, const = _read(e, d, dc, ns, k)
        assert np.array_equal(acc, G["acc"] + G2["acc"]) and np.array_equal(const, G["const"] + G2["const"])
        e.free(d)
        e.free(dc)
    # the text form: a line cut short, a line the frequency filter rejects, chromosome-X lines; the callback weighs by the ID field
    tcodes = codes.copy()
    tcodes[70] = 0x00
    tcodes[70, 5] = 0x01                                         # one alternate allele in the whole row: below the frequency filter
    lines = mg.text_of(tcodes).split(b"\n")[:-1]
    cut, on_x = [40, 299], [0, 63, 64, 150]
    text = b"".join((b"7\t5\trs" if i in cut else (b"X" + l[1:] if i in on_x else l)) + b"\n" for i, l in enumerate(lines))
    assert e.L.hpgv_set_text_filters(e.h, C.c_double(0.02), C.c_double(-1.0), C.c_long(-1)) == hpgv.OK
    calls = []

    def weigh(txt, n, line_off, field_off, status, wo, fo):
        calls.append(n)
        assert not wo.any() and not fo.any() and wo.shape == (n, k)
        for i in range(n):
            if (status[i] & 0xFF) == 1:
                continue
            head = txt[line_off[i]:line_off[i + 1]].split(b"\t")
            v = int(head[2][2:])                                 # "rs<v>"
            wo[i], fo[i] = w[v], flags[v]
        fo[on_x] &= ~np.uint8(sg.SKIP)                           # whatever the callback says, X lines are skipped
        return 0

    for impute in (0, 1):
        d, dc, ap = _zeroed(e, ns, k)
        rt = e.score_text(text, weigh, k, s, impute, d, ap, dc)
        acc, const = _read(e, d, dc, ns, k)
        assert rt["n_lines"] == nv and calls[-1] == nv
        filtered = (rt["status"] & LINE_FILTERED) != 0
        assert filtered[70] and not filtered[on_x].any()
        tskip = (filtered | np.isin(np.arange(nv), cut + on_x)).astype(np.uint8)
        G = sg.golden(tcodes, w, s, flags, impute, tskip)
        assert np.array_equal(acc, G["acc"]) and np.array_equal(const, G["const"]) and np.array_equal(rt["class4"], G["class4"])
        assert not rt["class4"][[0, 40, 63, 70]].any() and rt["class4"][1].any() and const[k] > nv // 2
        sg.check_acc(sg.run_dev(e, ig.lay(tcodes, pitch=pitch), ns, w, s, flags, impute, tskip), G)
        # more lines than room: n_lines says so, NOTHING was added and the callback was not invoked
        e.memset_dev(d, 0, (k + 2) * ap * 8)
        e.memset_dev(dc, 0, (k + 1) * 8)
        n_calls = len(calls)
        rt2 = e.score_text(text, weigh, k, s, impute, d, ap, dc, max_lines=nv - 10)
        acc, const = _read(e, d, dc, ns, k)
        assert rt2["n_lines"] > nv - 10 and not acc.any() and not const.any() and len(calls) == n_calls
        # a callback that refuses, and one that hands back a weight that is not finite: ERR_INVALID and nothing added
        for spoil in (lambda *a: 3, lambda t, n, lo, fo, st, wo, fl: wo.__setitem__((5, 1), np.inf)):
            with pytest.raises(hpgv.HpgvError):
                e.score_text(text, spoil, k, s, impute, d, ap, dc)
            acc, const = _read(e, d, dc, ns, k)
            assert not acc.any() and not const.any()
        e.free(d)
        e.free(dc)
    e.close()


def test_refusals(eng):
    d = eng.alloc(1 << 16)
    at = lambda off: C.c_void_p(d.value + off)
    s1 = np.zeros(32, np.int32)
    sp = hpgv._ptr(s1)
    cols = lambda gt, pitch, nv, nc, tab=at(8192), tp=64, ns=1, acc=at(4096), ap=64: eng.L.hpgv_score_cols_dev(eng.h, gt, pitch, nv, nc, None, tab, tp, ns, acc, ap, None)
    assert cols(d, 24, 4, 8) == hpgv.ERR_INVALID and cols(d, 0, 4, 0) == hpgv.ERR_INVALID                   # pitch
    assert cols(d, 16, 4, 17) == hpgv.ERR_INVALID and cols(d, 16, 4, -1) == hpgv.ERR_INVALID                # n_cols
    assert cols(d, 16, -1, 8) == hpgv.ERR_INVALID                                                           # n_variants
    assert cols(at(8), 16, 4, 8) == hpgv.ERR_INVALID                                                        # alignment
    assert cols(d, 16, 4, 8, at(8192 + 8)) == hpgv.ERR_INVALID and cols(d, 16, 4, 8, acc=at(4096 + 4)) == hpgv.ERR_INVALID
    assert cols(d, 16, 4, 8, tp=32) == hpgv.ERR_INVALID and cols(d, 16, 65, 8, tp=64) == hpgv.ERR_INVALID   # tab_pitch
    assert cols(d, 16, 4, 8, ns=0) == hpgv.ERR_INVALID and cols(d, 16, 4, 8, ns=33) == hpgv.ERR_INVALID     # n_scores
    assert cols(d, 16, 4, 8, ap=7) == hpgv.ERR_INVALID                                                      # acc_pitch
    assert cols(d, 16, 4, 8, None) == hpgv.ERR_INVALID and cols(d, 16, 4, 8, acc=None) == hpgv.ERR_INVALID and cols(None, 16, 4, 8) == hpgv.ERR_INVALID
    eng.h2d(d, np.full(1 << 14, 0x5A5A5A5A, np.int32))
    assert cols(d, 16, 4, 0) == hpgv.OK and cols(d, 16, 0, 8) == hpgv.OK and cols(None, 16, 0, 8, None, 0, 1, None) == hpgv.OK
    eng.sync()
    assert (eng.d2h(d, (1 << 14,), np.int32) == 0x5A5A5A5A).all()                                           # no column, no row: nothing written
    tab = lambda c4, nv, w=at(16384), fl=at(1024), ns=1, s=sp, skip=at(2048), t=at(8192), tp=64, cn=at(4096): eng.L.hpgv_score_table_dev(
        eng.h, c4, nv, w, fl, ns, s, 1, skip, t, tp, cn, None)
    assert tab(d, -1) == hpgv.ERR_INVALID
    assert tab(d, 4, ns=0) == hpgv.ERR_INVALID and tab(d, 4, ns=33) == hpgv.ERR_INVALID and tab(d, 4, s=None) == hpgv.ERR_INVALID
    for bad in (901, -901):
        assert tab(d, 4, s=hpgv._ptr(np.array([bad], np.int32))) == hpgv.ERR_INVALID
    assert tab(d, 4, tp=32) == hpgv.ERR_INVALID and tab(d, 65, tp=64) == hpgv.ERR_INVALID
    assert tab(at(8), 4) == hpgv.ERR_INVALID and tab(d, 4, t=at(8192 + 8)) == hpgv.ERR_INVALID
    assert tab(d, 4, w=at(16384 + 4)) == hpgv.ERR_INVALID and tab(d, 4, cn=at(4096 + 4)) == hpgv.ERR_INVALID
    for missing in ("w", "fl", "skip", "t", "cn"):
        assert tab(d, 4, **{missing: None}) == hpgv.ERR_INVALID
    assert tab(None, 4) == hpgv.ERR_INVALID
    assert tab(None, 0, None, None, 1, sp, None, None, 0, None) == hpgv.OK                                  # no rows, no table
    eng.sync()
    eng.free(d)


def test_state_and_group_refusals(cohort):
    codes = np.ascontiguousarray(cohort[:5])
    ns, k = codes.shape[1], 2
    text = mg.text_of(codes)
    nl = C.c_int(0)
    c4 = np.zeros((5, 4), np.int32)
    w, fl, s = np.ones((5, k)), np.zeros(5, np.uint8), np.zeros(k, np.int32)
    cb = hpgv.SCORE_WEIGH_FN(lambda *a: 0)
    e = hpgv.Engine(0)                                           # no stats cohort
    d, dc, ap = _zeroed(e, ns, k)
    P = hpgv._ptr
    host = lambda en=e, gt=P(codes), pitch=ns, nv=5, ww=P(w), ff=P(fl), kk=k, ss=P(s), cc=P(c4), acc=d, app=None, cn=dc: en.L.hpgv_score(
        en.h, gt, pitch, nv, ww, ff, kk, ss, 1, cc, acc, ap if app is None else app, cn)
    txt = lambda en=e, kk=k, ss=P(s), fn=cb, acc=d, cn=dc: en.L.hpgv_score_text(en.h, text, len(text), 5, C.byref(nl), None, None, None, fn, None, kk, ss, 1,
                                                                               P(c4), acc, ap, cn)
    assert host() == hpgv.ERR_STATE and txt() == hpgv.ERR_STATE
    e.set_stats_cohort(ns)
    assert host(pitch=ns - 1) == hpgv.ERR_INVALID and host(app=ns - 1) == hpgv.ERR_INVALID
    assert host(acc=C.c_void_p(d.value + 4)) == hpgv.ERR_INVALID and host(cn=C.c_void_p(dc.value + 4)) == hpgv.ERR_INVALID
    assert host(acc=None) == hpgv.ERR_INVALID and host(cn=None) == hpgv.ERR_INVALID and host(cc=None) == hpgv.ERR_INVALID
    assert host(ww=None) == hpgv.ERR_INVALID and host(ff=None) == hpgv.ERR_INVALID and host(gt=None) == hpgv.ERR_INVALID
    assert host(kk=0) == hpgv.ERR_INVALID and host(kk=33) == hpgv.ERR_INVALID and host(ss=None) == hpgv.ERR_INVALID
    assert txt(kk=0) == hpgv.ERR_INVALID and txt(kk=33) == hpgv.ERR_INVALID and txt(fn=hpgv.SCORE_WEIGH_FN()) == hpgv.ERR_INVALID
    for bad in (901, -901):
        sb = np.array([0, bad], np.int32)
        assert host(ss=P(sb)) == hpgv.ERR_INVALID and txt(ss=P(sb)) == hpgv.ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        wb = w.copy()
        wb[3, 1] = bad
        assert host(ww=P(wb)) == hpgv.ERR_INVALID
    assert host(gt=None, nv=0, ww=None, ff=None, cc=None) == hpgv.OK
    acc, const = _read(e, d, dc, ns, k)
    assert not acc.any() and not const.any()
    e.free(d)
    e.free(dc)
    e.close()
    g = hpgv.Engine([0, 0])
    assert g.L.hpgv_set_stats_cohort(g.h, ns) == hpgv.OK
    m = g.member(0)
    d, dc, ap = _zeroed(m, ns, k)
    assert host(en=g, acc=d, cn=dc) == hpgv.ERR_UNSUPPORTED and txt(en=g, acc=d, cn=dc) == hpgv.ERR_UNSUPPORTED
    # the device calls run on member 0, as the other *_dev calls do
    sg.check_acc(sg.run_dev(m, ig.lay(codes), ns, w, s, fl, 1), sg.golden(codes, w, s, fl, 1))
    m.free(d)
    m.free(dc)
    g.close()
