"""Goldens of the sample-relatedness counts (include/hpgv.h "IBS"), built in numpy from the code matrix: the pair counts from int64
indicator products over the rows, the class counts per row, the terms, E and the genome values in the header's operation order --
the sums over rows by a sequential Python loop, np.sum being pairwise --; and the helpers the tests share."""
import functools
import math
from fractions import Fraction

import numpy as np

from helpers import hpgv, random_codes
from model_golden import bits, classes

COLS = [1, 2, 17, 64, 65, 130]                         # no pair; one; a ragged wave; one whole tile; two tiles; three, the last ragged
ROWS = [1, 15, 64, 65, 300]                            # a ragged k-step; one whole; one and a row; five, the last ragged
SPLIT = (20, 5000)                                     # columns x rows: one tile pair, so the rows are cut into ranges


def indicators(codes, skip=None):
    """(valid, e0, e1, e2) int64 [rows, cols] with the skipped rows zeroed"""
    valid, g = classes(np.asarray(codes))
    keep = np.ones(len(codes), bool) if skip is None else np.asarray(skip) == 0
    v = (valid & keep[:, None]).astype(np.int64)
    return (v,) + tuple(v * (g == c) for c in range(3))


def pair_counts(codes, skip=None):
    """int64 [cols, cols, 4] = {n, ibs0, ibs1, ibs2} for i < j, zeros elsewhere"""
    v, e0, e1, e2 = indicators(codes, skip)
    n = v.T @ v
    ibs0 = e0.T @ e2 + e2.T @ e0
    ibs2 = e0.T @ e0 + e1.T @ e1 + e2.T @ e2
    out = np.stack([n, ibs0, n - ibs0 - ibs2, ibs2], axis=-1)
    out[~np.triu(np.ones(n.shape, bool), 1)] = 0
    return out


def class_counts(codes, skip=None):
    """int32 [rows, 4] = {n0, n1, n2, missing} over the columns, zeros for a skipped row"""
    v, e0, e1, e2 = indicators(codes, skip)
    out = np.stack([e0.sum(axis=1), e1.sum(axis=1), e2.sum(axis=1), codes.shape[1] - v.sum(axis=1)], axis=1).astype(np.int32)
    if skip is not None:
        out[np.asarray(skip) != 0] = 0
    return out


def fall(x, k):
    r = 1.0
    for t in range(k):
        r = r * (x - float(t))
    return r


def terms(n0, n1, n2):
    """(used, [t00, t01, t02, t11, t12]) in the header's operation order, Python floats (IEEE f64, no contraction)"""
    X, Y = 2 * int(n0) + int(n1), int(n1) + 2 * int(n2)
    if X + Y < 4:
        return False, [0.0] * 5
    x, y, t = float(X), float(Y), float(X + Y)
    F = lambda a, b: (fall(x, a) * fall(y, b)) / fall(t, a + b)
    return True, [2.0 * F(2, 2),
                  4.0 * F(3, 1) + 4.0 * F(1, 3),
                  (F(4, 0) + F(0, 4)) + 4.0 * F(2, 2),
                  2.0 * F(2, 1) + 2.0 * F(1, 2),
                  ((F(3, 0) + F(0, 3)) + F(2, 1)) + F(1, 2)]


def terms_exact(n0, n1, n2):
    """the same terms in rational arithmetic"""
    X, Y = 2 * int(n0) + int(n1), int(n1) + 2 * int(n2)
    T = X + Y
    ff = lambda x, k: math.prod(x - t for t in range(k))
    F = lambda a, b: Fraction(ff(X, a) * ff(Y, b), ff(T, a + b))
    return [2 * F(2, 2), 4 * F(3, 1) + 4 * F(1, 3), F(4, 0) + F(0, 4) + 4 * F(2, 2), 2 * F(2, 1) + 2 * F(1, 2), F(3, 0) + F(0, 3) + F(2, 1) + F(1, 2)]


def expected(class4):
    """(E [5] float64, used rows): the used rows' terms added sequentially in row order, divided by their number"""
    total, m = [0.0] * 5, 0
    for n0, n1, n2 in np.asarray(class4)[:, :3].tolist():
        used, t = terms(n0, n1, n2)
        if used:
            m += 1
            total = [a + b for a, b in zip(total, t)]
    with np.errstate(invalid="ignore"):
        return np.array(total, np.float64) / np.float64(m), m


def genome(c, E):
    """[Z0, Z1, Z2, PI_HAT, DST] of one record {n, ibs0, ibs1, ibs2} in the header's order; numpy f64 scalars, so that a division by
    zero gives the IEEE value"""
    f = np.float64
    E00, E01, E02, E11, E12 = (f(x) for x in E)
    S, i0, i1, i2 = (f(int(x)) for x in c)
    with np.errstate(all="ignore"):
        z0 = i0 / (E00 * S)
        z1 = (i1 - z0 * (E01 * S)) / (E11 * S)
        z2 = (i2 - z0 * (E02 * S) - z1 * (E12 * S)) / S
        if z0 > 1:
            z0, z1, z2 = f(1), f(0), f(0)
        if z1 > 1:
            z0, z1, z2 = f(0), f(1), f(0)
        if z2 > 1:
            z0, z1, z2 = f(0), f(0), f(1)
        if z0 < 0:
            t = z1 + z2
            z0, z1, z2 = f(0), z1 / t, z2 / t
        if z1 < 0:
            t = z0 + z2
            z0, z1, z2 = z0 / t, f(0), z2 / t
        if z2 < 0:
            t = z0 + z1
            z0, z1, z2 = z0 / t, z1 / t, f(0)
        return np.array([z0, z1, z2, z1 / f(2) + z2, (i2 + f(0.5) * i1) / S], np.float64)


def genome_all(counts, E):
    """genome() of every record of an int [..., 4] array"""
    c = np.asarray(counts).reshape(-1, 4)
    return np.array([genome(r, E) for r in c.tolist()], np.float64).reshape(np.asarray(counts).shape[:-1] + (5,))


def selected(pi_hat, min_pi_hat):
    """the golden list of hpgv_ibs_select_dev from the PI_HAT matrix of genome_all: (i, j, pi_hat) of the pairs i < j with
    PI_HAT >= min_pi_hat (a NaN never is), sorted by (i, j)"""
    with np.errstate(invalid="ignore"):
        hit = np.triu(pi_hat >= min_pi_hat, 1)
    return [(int(i), int(j), pi_hat[i, j]) for i, j in np.argwhere(hit)]


def same_bits(got, exp, what=""):
    """NaN in the same places and bit for bit equal elsewhere (which NaN is not defined)"""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN pattern differs" % what
    assert np.array_equal(bits(got)[~nan], bits(exp)[~nan]), "%s: bits differ" % what


@functools.lru_cache(maxsize=None)
def matrix(rows, cols):
    """random codes [rows, cols]; read-only, shared by the tests"""
    rng = np.random.default_rng(4200 + 1000 * cols + rows)
    codes = random_codes(rng, rows, cols, quirks=True, strict=False)
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def golden(rows, cols):
    out = pair_counts(matrix(rows, cols))
    out.setflags(write=False)
    return out


def lay(codes, pitch=None, fill=0xFF, seed=1):
    """a code matrix as a device matrix of `pitch` bytes per row (default: the next multiple of 16 with at least one pad column);
    the columns past the codes hold `fill`, or random bytes for fill=None"""
    rows, cols = codes.shape
    if pitch is None:
        pitch = (cols // 16 + 1) * 16
    if fill is None:
        out = np.random.default_rng(seed).integers(0, 256, (rows, pitch), dtype=np.uint8)
    else:
        out = np.full((rows, pitch), fill, np.uint8)
    out[:, :cols] = codes
    return out


PATTERN = 0x5A5A5A5A


def fresh_counts(n_cols):
    """the caller's buffer before the first call: zeros for i < j, a pattern elsewhere -- which must come back unchanged"""
    buf = np.full((n_cols, n_cols, 4), PATTERN, np.int32)
    buf[np.triu(np.ones((n_cols, n_cols), bool), 1)] = 0
    return buf


def check_counts(got, exp, what=""):
    """the counts where i < j, the pattern elsewhere"""
    nc = got.shape[0]
    upper = np.triu(np.ones((nc, nc), bool), 1)
    assert (got[~upper] == PATTERN).all(), "%s: an element with i >= j was touched" % what
    bad = np.argwhere((got[upper] != exp[upper]).any(axis=-1))
    assert len(bad) == 0, "%s: counts differ at %s" % (what, np.argwhere(upper)[bad[:4, 0]].tolist())


class DevCounts:
    """a counts buffer on the device for a run of calls"""

    def __init__(self, e, n_cols):
        self.e, self.n_cols = e, n_cols
        self.d = e.alloc(max(n_cols * n_cols * 16, 16))
        e.h2d(self.d, fresh_counts(n_cols))

    def get(self):
        self.e.sync()
        return self.e.d2h(self.d, (self.n_cols, self.n_cols, 4), np.int32)

    def close(self):
        self.e.free(self.d)


def add_dev(e, dc, laid, n_cols, skip=None):
    """hpgv_ibs_pairs_dev of a laid-out matrix into a DevCounts"""
    laid = np.ascontiguousarray(laid, np.uint8)
    nv, pitch = laid.shape
    d_gt = e.alloc(max(laid.nbytes, 16))
    e.h2d(d_gt, laid)
    d_skip = None
    if skip is not None:
        d_skip = e.alloc(max(nv, 16))
        e.h2d(d_skip, np.asarray(skip, np.uint8))
    e.ibs_pairs_dev(d_gt, pitch, nv, n_cols, dc.d, d_skip=d_skip)
    e.sync()
    e.free(d_gt)
    if d_skip is not None:
        e.free(d_skip)


def run_dev(e, laid, n_cols, skip=None):
    """one call into a fresh buffer: the whole [n_cols, n_cols, 4] buffer"""
    dc = DevCounts(e, n_cols)
    add_dev(e, dc, laid, n_cols, skip)
    out = dc.get()
    dc.close()
    return out


def class_dev(e, laid, n_cols, skip=None):
    """hpgv_ibs_class_counts_dev: [rows, 4], the output filled with a pattern first"""
    laid = np.ascontiguousarray(laid, np.uint8)
    nv, pitch = laid.shape
    d_gt, d_c4 = e.alloc(max(laid.nbytes, 16)), e.alloc(nv * 16)
    e.h2d(d_gt, laid)
    e.h2d(d_c4, np.full((nv, 4), PATTERN, np.int32))
    d_skip = None
    if skip is not None:
        d_skip = e.alloc(max(nv, 16))
        e.h2d(d_skip, np.asarray(skip, np.uint8))
    e.ibs_class_counts_dev(d_gt, pitch, nv, n_cols, d_c4, d_skip=d_skip)
    e.sync()
    out = e.d2h(d_c4, (nv, 4), np.int32)
    for b in (d_gt, d_c4) + (() if d_skip is None else (d_skip,)):
        e.free(b)
    return out


def engine():
    return hpgv.Engine(0)
