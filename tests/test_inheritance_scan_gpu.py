"""hpgv_inheritance_scan_dev: the counts behind --inh-dom / --inh-rec on HPGV_LAYOUT_ASSOC rows, count for count against
numpy, and the verdicts hpgv_filter_text ORs into the line status (include/hpgv.h hpgv_set_text_inheritance_filters)."""
import ctypes as C

import numpy as np
import pytest

from helpers import hpgv

pytestmark = pytest.mark.gpu

LINE_FILTERED = 0x100                                          # include/hpgv.h HPGV_LINE_FILTERED
CODES = np.array([0x00, 0x01, 0x10, 0x11, 0x12, 0x22, 0xE1, 0x0F, 0xF0, 0xFF], np.uint8)


def model(raw, cond):
    """the eight counts per variant of the raw matrix (VCF column order) under the condition vector"""
    g = raw.astype(np.int32)
    counted = ((g >> 4) != 0xF) & ((g & 0xF) != 0xF)
    nonref = counted & (g != 0)
    both = counted & ((g >> 4) != 0) & ((g & 0xF) != 0)
    A, U = cond == hpgv.COND_AFFECTED, cond == hpgv.COND_UNAFFECTED
    out = np.zeros((raw.shape[0], 8), np.int32)
    out[:, 0] = counted[:, A].sum(1); out[:, 1] = nonref[:, A].sum(1); out[:, 2] = both[:, A].sum(1)
    out[:, 3] = counted[:, U].sum(1); out[:, 4] = (counted & (g == 0))[:, U].sum(1); out[:, 5] = both[:, U].sum(1)
    return out


def scan(e, raw, cond):
    nv, ns = raw.shape
    e.set_cohort(cond)
    pitch_raw = max(16, (ns + 15) // 16 * 16)
    src = np.full((nv, pitch_raw), 0xFF, np.uint8)
    src[:, :ns] = raw
    _, _, pitch = e.assoc_layout()
    d_raw, d_lay, d_c8 = e.alloc(src.nbytes), e.alloc(nv * pitch), e.alloc(nv * 32)
    e.h2d(d_raw, src)
    e.layout(hpgv.LAYOUT_ASSOC, d_raw, pitch_raw, nv, d_lay)
    e.inheritance_scan(d_lay, nv, d_c8)
    e.sync()
    got = e.d2h(d_c8, (nv, 8), np.int32)
    for p in (d_raw, d_lay, d_c8):
        e.free(p)
    return got


def cohort(rng, n_aff, n_unaff, n_other):
    cond = np.array([hpgv.COND_AFFECTED] * n_aff + [hpgv.COND_UNAFFECTED] * n_unaff + [hpgv.COND_OTHER] * n_other, np.uint8)
    return cond[rng.permutation(len(cond))]


@pytest.mark.parametrize("n_aff", [0, 1, 15, 16, 17])
@pytest.mark.parametrize("n_unaff", [0, 1, 15, 16, 17])
def test_class_sizes_and_codes(n_aff, n_unaff):
    rng = np.random.default_rng(100 * n_aff + n_unaff)
    cond = cohort(rng, n_aff, n_unaff, 5)
    nv = 301
    raw = CODES[rng.integers(0, len(CODES), (nv, len(cond)))]
    raw[0, :] = 0x11; raw[1, :] = 0x00; raw[2, :] = 0xFF; raw[3, :] = 0x0F            # whole rows of one code
    e = hpgv.Engine(0)
    try:
        assert np.array_equal(scan(e, raw, cond), model(raw, cond))
    finally:
        e.close()


def test_every_code_in_every_class():
    rng = np.random.default_rng(3)
    cond = cohort(rng, 40, 37, 11)
    raw = np.repeat(CODES, 9)[:, None].repeat(len(cond), 1)                               # one code per row
    raw = np.concatenate([raw, CODES[rng.integers(0, len(CODES), (200, len(cond)))]])
    e = hpgv.Engine(0)
    try:
        got = scan(e, raw, cond)
        assert np.array_equal(got, model(raw, cond))
        # spot values: 0xE1 counts as non-reference and both; 0x0F / 0xF0 are not counted
        k = int(np.where(CODES == 0xE1)[0][0]) * 9
        assert tuple(got[k, :6]) == (40, 40, 40, 37, 0, 37)
        k = int(np.where(CODES == 0x0F)[0][0]) * 9
        assert tuple(got[k]) == (0,) * 8
        k = int(np.where(CODES == 0x10)[0][0]) * 9
        assert tuple(got[k, :6]) == (40, 40, 0, 37, 0, 0)
    finally:
        e.close()


def test_seventy_thousand_affected():
    """per-lane partial sums packed in 16-bit halves must not overflow with 65 536 or more samples in one class"""
    rng = np.random.default_rng(5)
    cond = cohort(rng, 70000, 1500, 300)
    nv = 24
    raw = CODES[rng.integers(0, len(CODES), (nv, len(cond)))]
    raw[0, :] = 0x11; raw[1, :] = 0x00; raw[2, :] = 0x12
    e = hpgv.Engine(0)
    try:
        got = scan(e, raw, cond)
        exp = model(raw, cond)
        assert np.array_equal(got, exp)
        assert tuple(got[0, :3]) == (70000, 70000, 70000) and got[1, 0] == 70000 and got[1, 1] == 0
    finally:
        e.close()


def test_group_context_gives_the_same_counts():
    rng = np.random.default_rng(8)
    cond = cohort(rng, 333, 290, 20)
    raw = CODES[rng.integers(0, len(CODES), (517, len(cond)))]
    e, g = hpgv.Engine(0), hpgv.Engine([0, 0])
    try:
        one = scan(e, raw, cond)
        assert np.array_equal(scan(g, raw, cond), one)
        assert np.array_equal(one, model(raw, cond))
    finally:
        g.close(); e.close()


def test_scan_without_a_cohort_is_a_state_error():
    e = hpgv.Engine(0)
    try:
        d = e.alloc(1024)
        rc = e.L.hpgv_inheritance_scan_dev(e.h, d, 1, d, None)
        assert rc == hpgv.ERR_STATE
        assert e.L.hpgv_set_text_inheritance_filters(e.h, 1.5, -1.0) == hpgv.ERR_INVALID
        assert e.L.hpgv_set_text_inheritance_filters(e.h, -1.0, 1.0000001) == hpgv.ERR_INVALID
    finally:
        e.close()


# ---- the verdicts of the text path -------------------------------------------------------------------------------------
GT_TEXT = {0x00: "0/0", 0x01: "0/1", 0x10: "1/0", 0x11: "1/1", 0x12: "1/2", 0x22: "2/2", 0xFF: "./.", 0x0F: "0/."}


def _text(raw):
    lines = []
    for v in range(raw.shape[0]):
        lines.append("1\t%d\trs%d\tA\tC,G\t50\tPASS\t.\tGT\t%s\n" % (100 + v, v, "\t".join(GT_TEXT[int(c)] for c in raw[v])))
    return "".join(lines).encode()


def _filter_text(e, text, max_lines):
    L = e.L
    L.hpgv_filter_text.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]
    L.hpgv_text_partition.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    buf = C.create_string_buffer(text, len(text))
    line_off = np.zeros(max_lines + 1, np.uint64)
    field_off = np.zeros(10 * max_lines, np.uint32)
    status = np.zeros(max_lines, np.int32)
    nl = C.c_int()
    rc = L.hpgv_filter_text(e.h, C.cast(buf, C.c_char_p), len(text), max_lines, C.byref(nl), line_off.ctypes.data, field_off.ctypes.data,
                            status.ctypes.data)
    L.hpgv_text_partition(e.h, C.cast(buf, C.c_char_p), None, 0, None, 0, None, None)         # the hold released
    return rc, nl.value, status


@pytest.mark.parametrize("dom,rec", [(0.5, -1.0), (-1.0, 0.5), (0.75, 0.25), (0.0, -1.0), (1.0, 1.0)])
def test_filter_text_status_against_numpy_fractions(dom, rec):
    rng = np.random.default_rng(int((dom + 2) * 100 + (rec + 2) * 10))
    cond = cohort(rng, 6, 2, 2)
    codes = np.array(list(GT_TEXT), np.uint8)
    raw = codes[rng.integers(0, len(codes), (400, len(cond)))]
    raw[0, :] = 0xFF                                            # no counted call: fails
    # fractions exactly at the thresholds: 6 affected 0/1, unaffected 0/0 and 1/1 -> dominant 7 / 8, recessive 1 / 8 ...
    aff, una = np.where(cond == hpgv.COND_AFFECTED)[0], np.where(cond == hpgv.COND_UNAFFECTED)[0]
    raw[1, :] = 0x00; raw[1, aff[:4]] = 0x01; raw[1, aff[4:]] = 0x11                   # dominant 4+2 ... /8
    raw[2, :] = 0x11; raw[2, aff[:2]] = 0x00                                          # recessive (4 + 2 - 2) / 8 = 0.5
    raw[3, :] = 0x00; raw[3, aff[:3]] = 0x01; raw[3, una[:1]] = 0xFF                  # dominant (3 + 1) / 7 ...
    raw[4, :] = 0x00; raw[4, aff[:2]] = 0x01; raw[4, aff[2:4]] = 0x0F; raw[4, aff[4:]] = 0xFF   # dominant (2 + 2) / 4 = 1
    raw[5, :] = 0x00; raw[5, aff[:2]] = 0x01; raw[5, una] = 0x11; raw[5, aff[2:]] = 0x0F          # dominant 2 / 4 = 0.5
    e = hpgv.Engine(0)
    try:
        e.set_stats_cohort(len(cond))
        e.set_cohort(cond)
        e.set_text_inheritance_filters(dom, rec)
        text = _text(raw)
        rc, nl, status = _filter_text(e, text, raw.shape[0])
        assert rc == 0, e.L.hpgv_last_error(e.h)
        assert nl == raw.shape[0]
        c = model(np.where(((raw >> 4) == 0xF) | ((raw & 0xF) == 0xF), 0xFF, raw).astype(np.uint8), cond).astype(np.int64)
        den = c[:, 0] + c[:, 3]
        keep = den > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            fd = (c[:, 1] + c[:, 4]) / den
            fr = (c[:, 2] + (c[:, 3] - c[:, 5])) / den
        if dom >= 0: keep &= fd >= dom
        if rec >= 0: keep &= fr >= rec
        got_keep = (status & LINE_FILTERED) == 0
        assert np.array_equal(got_keep, keep)
        assert not got_keep[0]
        exact = (dom >= 0 and np.any(fd[keep] == dom)) or (rec >= 0 and np.any(fr[keep] == rec))
        if (dom, rec) in ((0.5, -1.0), (-1.0, 0.5)):
            assert exact                                         # a fraction exactly at the threshold is kept
        # switched off again: every line with a counted call passes; the filter needs the cohort over the same columns
        e.set_text_inheritance_filters(-1.0, -1.0)
        rc, nl, status = _filter_text(e, text, raw.shape[0])
        assert rc == 0 and not np.any(status & LINE_FILTERED)
        e.set_text_inheritance_filters(dom, rec)
        e.set_cohort(np.concatenate([cond, [hpgv.COND_AFFECTED]]).astype(np.uint8))
        rc, _, _ = _filter_text(e, text, raw.shape[0])
        assert rc == hpgv.ERR_STATE
    finally:
        e.close()
