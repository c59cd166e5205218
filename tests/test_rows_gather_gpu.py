"""hpgv_rows_gather_dev (the kept rows of a matrix, compacted on the device) against numpy -- destination, index array and count
exact, every byte that is no kept row's untouched -- and hpgv_assoc_select_text: hpgv_assoc_text's outputs bit for bit, plus the
candidate lines (a record, not filtered, p <= p_max) numbered and their genotype rows gathered."""
import ctypes as C

import numpy as np
import pytest

from helpers import hpgv
from oracle import pyoracle as orc
from test_gpu_text import _line

pytestmark = pytest.mark.gpu

GUARD = 0xC3
LINE_FILTERED = 0x100                                            # HPGV_LINE_FILTERED of include/hpgv.h


@pytest.fixture(scope="module")
def eng():
    e = hpgv.Engine(0)
    yield e
    e.close()


def _keeps(rng, n):
    every_other = (np.arange(n) % 2).astype(np.uint8)
    some = (rng.random(n) < 0.3).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)     # any non-zero byte keeps
    return dict(none=np.zeros(n, np.uint8), all=np.ones(n, np.uint8), every_other=every_other, random=some)


def _gather(e, src, row_bytes, keep, dst_pitch, src_shift=0, dst_shift=0):
    """the call on device copies: (the whole destination block with its guard bytes, index, n_kept).  src: [n, src_pitch]; the
    shifts move the two matrices off their 16-byte alignment"""
    n, src_pitch = src.shape
    dst_rows = n + 1                                              # one row of guard behind the last possible row
    bufs = [e.alloc(max(src.size, 1) + 32), e.alloc(dst_rows * dst_pitch + 32), e.alloc(max(n, 1) + 16), e.alloc(4 * n + 16), e.alloc(16),
            e.alloc(e.rows_gather_scratch_bytes(n))]
    d_src, d_dst, d_keep, d_index, d_count, d_scratch = bufs
    at = lambda d, k: C.c_void_p(d.value + k)
    if n:
        e.h2d(at(d_src, src_shift), np.ascontiguousarray(src))
        e.h2d(d_keep, keep)
        e.h2d(d_index, np.full(n, -7, np.int32))
    e.h2d(at(d_dst, dst_shift), np.full(dst_rows * dst_pitch, GUARD, np.uint8))
    e.h2d(d_count, np.array([-7], np.int32))
    e.rows_gather_dev(at(d_src, src_shift), src_pitch, row_bytes, n, d_keep, at(d_dst, dst_shift), dst_pitch, d_index, d_count, d_scratch)
    e.sync()
    dst = e.d2h(at(d_dst, dst_shift), (dst_rows, dst_pitch), np.uint8)
    index = e.d2h(d_index, (n,), np.int32) if n else np.zeros(0, np.int32)
    count = int(e.d2h(d_count, (1,), np.int32)[0])
    for b in bufs:
        e.free(b)
    return dst, index, count


@pytest.mark.parametrize("row_bytes", [5, 16, 82, 713])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300])
def test_gather(eng, n, row_bytes):
    rng = np.random.default_rng(1000 * n + row_bytes)
    al = -(-row_bytes // 16) * 16
    # both aligned (the 16-byte path); the source pitch odd; the destination pitch odd; aligned pitches at shifted pointers
    for src_pitch, dst_pitch, src_shift, dst_shift in ((al + 16, al, 0, 0), (row_bytes + 3, al, 0, 0), (al, row_bytes + 1, 0, 0), (al, al + 16, 4, 0),
                                                       (al, al, 0, 9), (row_bytes, row_bytes, 0, 0)):
        src = rng.integers(0, 256, (n, src_pitch), dtype=np.uint8)
        for name, keep in _keeps(rng, n).items():
            dst, index, count = _gather(eng, src, row_bytes, keep, dst_pitch, src_shift, dst_shift)
            kept = np.flatnonzero(keep)
            what = (name, src_pitch, dst_pitch, src_shift, dst_shift)
            assert count == len(kept), what
            exp_index = np.full(n, -1, np.int32)
            exp_index[kept] = np.arange(len(kept))
            assert np.array_equal(index, exp_index), what
            exp = np.full((n + 1, dst_pitch), GUARD, np.uint8)
            exp[:len(kept), :row_bytes] = src[kept, :row_bytes]
            assert np.array_equal(dst, exp), (what, np.argwhere(dst != exp)[:4].tolist())


def test_gather_refusals(eng):
    d = eng.alloc(4096)
    at = lambda k: C.c_void_p(d.value + k)
    call = lambda src_pitch=16, row_bytes=16, n=4, keep=at(512), dst_pitch=16, index=at(1024), count=at(2048), scratch=at(3072): \
        eng.L.hpgv_rows_gather_dev(eng.h, d, src_pitch, row_bytes, n, keep, at(256), dst_pitch, index, count, scratch, None)
    assert call(n=-1) == hpgv.ERR_INVALID and call(src_pitch=8) == hpgv.ERR_INVALID and call(dst_pitch=15) == hpgv.ERR_INVALID
    assert call(keep=None) == hpgv.ERR_INVALID and call(index=None) == hpgv.ERR_INVALID and call(count=None) == hpgv.ERR_INVALID
    assert call(scratch=None) == hpgv.ERR_INVALID and call(scratch=at(3076)) == hpgv.ERR_INVALID
    eng.h2d(at(512), np.zeros(4, np.uint8))
    assert call() == hpgv.OK and call(n=0, keep=None, index=None, scratch=None) == hpgv.OK
    eng.sync()
    eng.free(d)


# ---- hpgv_assoc_select_text ----------------------------------------------------------------------------------------------

N_SAMPLES, N_LINES = 90, 120
HEADER, DAMAGED, FILTERED = 0, 41, 77


def _text():
    """120 lines for 90 samples: a header line, a line cut short, and a line with a strong signal that the missing-rate filter
    rejects; every tenth line carries a signal, so the p-values spread over many decades"""
    rng = np.random.default_rng(77)
    cond = rng.permutation(np.array([1] * 40 + [0] * 40 + [2] * 10, np.uint8))
    names = np.array(["0/0", "0/1", "1/1", "./."])
    lines = []
    for i in range(N_LINES):
        freq = np.where((cond == 1) & (i % 10 == 7), 0.65, 0.3)
        g = rng.binomial(2, freq)
        miss = rng.random(N_SAMPLES) < (0.4 if i == FILTERED else 0.03)
        lines.append(_line(rng, N_SAMPLES, "GT", "7", gts=names[np.where(miss, 3, g)].tolist()))
    lines[HEADER] = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("s%d" % j for j in range(N_SAMPLES))
    lines[DAMAGED] = "7\t5\trs"
    return ("\n".join(lines) + "\n").encode(), cond


def _engine(path, monkeypatch):
    """the three ways hpgv_assoc_text counts a text: k_assoc_rows, the fused per-row kernel, the layout and the scans' chain"""
    monkeypatch.setenv("HPGV_ASSOC_ROWS", "1" if path == "rows" else "0")
    e = hpgv.Engine(0)
    if path == "chain":
        e.set_option("batch_fused", 0)
    return e


@pytest.mark.parametrize("path", ["rows", "fused", "chain"])
def test_assoc_select_text(path, monkeypatch):
    text, cond = _text()
    e = _engine(path, monkeypatch)
    e.set_cohort(cond)
    assert e.L.hpgv_set_stats_cohort(e.h, N_SAMPLES) == hpgv.OK
    assert e.L.hpgv_set_text_filters(e.h, C.c_double(-1.0), C.c_double(0.2), C.c_long(-1)) == hpgv.OK
    e.set_logfact(orc.logfact(N_SAMPLES * 10))
    raw = orc.tokenize(text.decode(), N_SAMPLES, False)["gt"]       # the raw matrix: half-called genotypes kept
    for task in (hpgv.TASK_CHISQ, hpgv.TASK_FISHER):
        base = e.assoc_text(task, text)
        st, p = base["status"], base["p"]
        assert base["n_lines"] == N_LINES
        assert (st[HEADER] & 0xFF) != 0 and (st[DAMAGED] & 0xFF) != 0 and st[FILTERED] == LINE_FILTERED
        usable = ((st & 0xFF) == 0) & ((st & LINE_FILTERED) == 0)
        assert usable.sum() == N_LINES - 3
        ps = np.sort(p[usable & ~np.isnan(p)])
        k = len(ps) // 3
        assert ps[k - 1] < ps[k]
        mid = 0.5 * (ps[k - 1] + ps[k])
        assert p[FILTERED] < mid, "the filtered line would be a candidate by its p"
        for p_max, n_exp in ((mid, k), (float(ps[k]), k + 1 + int((ps[k + 1:] == ps[k]).sum())), (1.0, len(ps)), (0.0, int((ps == 0).sum()))):
            with np.errstate(invalid="ignore"):
                keep = usable & (p <= p_max)
            assert keep.sum() == n_exp
            exp_sel = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
            got = e.assoc_select_text(task, text, p_max, rows_pitch=N_SAMPLES + 6)
            assert got["n_lines"] == N_LINES and got["n_sel"] == n_exp
            assert np.array_equal(got["sel"], exp_sel)
            assert np.array_equal(got["rows"], raw[keep])
            block = got["rows_block"]
            assert (block[:, N_SAMPLES:] == 0xEE).all() and (block[n_exp:] == 0xEE).all(), "bytes outside the candidate rows were written"
            for key in ("status", "A1", "A2", "U1", "U2"):
                assert np.array_equal(got[key], base[key]), key
            for key in ("odds", "chisq", "p"):
                if base[key] is not None:
                    assert np.array_equal(got[key].view(np.uint64), base[key].view(np.uint64)), key
            # too little room: the count and sel as before, no row copied
            if n_exp > 0:
                small = e.assoc_select_text(task, text, p_max, rows_cap=n_exp - 1)
                assert small["n_sel"] == n_exp and small["rows"] is None and np.array_equal(small["sel"], exp_sel)
                assert (small["rows_block"] == 0xEE).all()
                exact = e.assoc_select_text(task, text, p_max, rows_cap=n_exp)
                assert np.array_equal(exact["rows"], raw[keep])
    # fewer lines of room than the text has; no text; refusals
    short = e.assoc_select_text(hpgv.TASK_CHISQ, text, 1.0, max_lines=50)
    full = e.assoc_text(hpgv.TASK_CHISQ, text, max_lines=50)
    keep = ((full["status"] & 0xFF) == 0) & ((full["status"] & LINE_FILTERED) == 0) & ~np.isnan(full["p"])
    assert short["n_lines"] == N_LINES and len(short["sel"]) == 50 and short["n_sel"] == keep.sum() and np.array_equal(short["rows"], raw[:50][keep])
    assert e.assoc_select_text(hpgv.TASK_CHISQ, b"", 1.0)["n_sel"] == 0
    with pytest.raises(hpgv.HpgvError):
        e.assoc_select_text(hpgv.TASK_CHISQ, text, float("nan"))
    with pytest.raises(hpgv.HpgvError):
        e.assoc_select_text(hpgv.TASK_CHISQ, text, 0.5, rows_pitch=N_SAMPLES - 1)
    e.close()


def test_assoc_select_text_on_a_group_context(monkeypatch):
    text, cond = _text()
    g = hpgv.Engine([0, 0])
    g.set_cohort(cond)
    one = hpgv.Engine(0)
    one.set_cohort(cond)
    a, b = g.assoc_select_text(hpgv.TASK_CHISQ, text, 0.01), one.assoc_select_text(hpgv.TASK_CHISQ, text, 0.01)
    assert a["n_sel"] == b["n_sel"] > 0 and np.array_equal(a["sel"], b["sel"]) and np.array_equal(a["rows"], b["rows"])
    assert np.array_equal(a["p"].view(np.uint64), b["p"].view(np.uint64))
    g.close(), one.close()
