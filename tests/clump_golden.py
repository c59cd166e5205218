"""Goldens of the LD edge form and of clumping (include/hpgv.h "LD", hpgv_clump), built from ld_golden's numpy band: the edge set
is the band's pairs with r2 >= min_r2, and the clump assignment is a direct Python loop over candidates and edges.  Nothing here
calls the code under test but run_edges, the helper that launches it."""
import functools
import math

import numpy as np

import ld_golden as lg
from helpers import hpgv, random_codes
from model_golden import bits

EDGE = np.dtype([("a", np.int32), ("b", np.int32), ("r2", np.float64)])     # hpgv_ld_edge
GUARD = 8                                                                  # records behind edge_cap that must keep their pattern
PATTERN = 0xA5


def edges_of_band(r2, min_r2, b_begin=0):
    """the pairs (b - d, b) of a band r2 [nv - b_begin, window] with r2 >= min_r2 (NaN never is), sorted by (b, a)"""
    with np.errstate(invalid="ignore"):
        rows, cols = np.nonzero(r2 >= min_r2)
    out = np.zeros(len(rows), EDGE)
    out["b"] = rows + b_begin
    out["a"] = out["b"] - (cols + 1)
    out["r2"] = r2[rows, cols]
    return np.sort(out, order=("b", "a"))


def sort_edges(e):
    return np.sort(np.asarray(e, EDGE), order=("b", "a"))


def assert_edges_equal(got, exp, what=""):
    """(a, b) exact and r2 bit for bit, both lists sorted by (b, a)"""
    assert len(got) == len(exp), "%s: %d edges, expected %d" % (what, len(got), len(exp))
    assert np.array_equal(got["a"], exp["a"]) and np.array_equal(got["b"], exp["b"]), "%s: pairs differ" % what
    assert np.array_equal(bits(got["r2"]), bits(exp["r2"])), "%s: r2 bits differ" % what


def median_r2(r2):
    """the median of the finite r2 of a band, 0.5 where there is none"""
    f = r2[np.isfinite(r2)]
    return float(np.median(f)) if len(f) else 0.5


@functools.lru_cache(maxsize=None)
def planted(width, nv):
    """ld_golden.matrix with planted partners: every fifth row from row 3 on is an earlier row (1 to 3 rows back, so inside every
    window) turned by ld_golden.flip (r2 = 1) or copied with 5 % of its bytes redrawn (r2 high), in turn"""
    rng = np.random.default_rng(9300 + 100 * width[0] + nv)
    codes = lg.matrix(width, nv, quirks=False).copy()
    ns = codes.shape[1]
    for k, j in enumerate(range(3, nv, 5)):
        src = codes[j - 1 - k % 3]
        if k % 2 == 0:
            codes[j] = lg.flip(src)
        else:
            redraw = rng.random(ns) < 0.05
            codes[j] = np.where(redraw, random_codes(rng, 1, ns, quirks=False, strict=False)[0], src)
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def planted_golden(width, nv, window):
    out = lg.band(planted(width, nv), window)
    for a in out:
        a.setflags(write=False)
    return out


def run_edges(e, laid, window, min_r2, cap=None, b_begin=0, chrom=None, pos=None, max_bp=-1, skip=None, counter_pattern=0x5A5A5A5A5A5A5A5A):
    """hpgv_ld_edges_dev on a laid-out matrix.  cap None: a list with room for the whole band.  Returns (the stored records sorted
    by (b, a), the count the call left, whether the GUARD records behind `cap` kept their pattern).  cap 0 passes d_edges = NULL.
    The counter is filled with a pattern first: the call is to overwrite it"""
    laid = np.ascontiguousarray(laid, np.uint8)
    nv, pitch = laid.shape
    if cap is None:
        cap = max(nv - b_begin, 0) * window
    bufs = []

    def up(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        d = e.alloc(max(a.nbytes, 16))
        bufs.append(d)
        if a.nbytes:
            e.h2d(d, a)
        return d
    d_gt = up(laid)
    d_chrom = up(None if chrom is None else np.asarray(chrom, np.int32))
    d_pos = up(None if pos is None else np.asarray(pos, np.uint32))
    d_skip = up(None if skip is None else np.asarray(skip, np.uint8))
    d_edges = up(np.full((cap + GUARD) * EDGE.itemsize, PATTERN, np.uint8))
    d_n = up(np.array([counter_pattern], np.uint64))
    e.ld_edges_dev(d_gt, pitch, nv, window, min_r2, d_edges if cap else None, cap, d_n, b_begin=b_begin, d_chrom=d_chrom, d_pos=d_pos,
                   max_bp=max_bp, d_skip=d_skip)
    e.sync()
    count = int(e.d2h(d_n, (1,), np.uint64)[0])
    raw = e.d2h(d_edges, ((cap + GUARD) * EDGE.itemsize,), np.uint8)
    for b in bufs:
        e.free(b)
    stored = raw[:min(count, cap) * EDGE.itemsize].view(EDGE)
    guard_ok = bool((raw[min(count, cap) * EDGE.itemsize:] == PATTERN).all())
    return sort_edges(stored), count, guard_ok


def clump_loop(p, pairs, p1):
    """PLINK's default --clump as a direct loop: (index_of, clump_order).  pairs: (a, b) candidate numbers, undirected"""
    n = len(p)
    index_of = [-1] * n
    order = []
    for i in sorted((i for i in range(n) if not math.isnan(p[i])), key=lambda i: (p[i], i)):
        if p[i] > p1:
            break
        if index_of[i] != -1:
            continue
        index_of[i] = i
        order.append(i)
        for a, b in pairs:
            for x, y in ((a, b), (b, a)):
                if x == i and index_of[y] == -1:
                    index_of[y] = i
    return np.array(index_of, np.int32), np.array(order, np.int32)
