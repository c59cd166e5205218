"""Goldens of the genetic relationship matrix (include/hpgv.h "GRM"), built in numpy from the code matrix: the rows' tables in the
header's operation order with np.rint, the pair sums from int64 products Q.T @ Q and V.T @ V over the used rows, the value, the
three files of the runner; and the helpers the tests share."""
import functools

import numpy as np

import ibs_golden as ig
from helpers import hpgv
from model_golden import classes

MAX_Q = 127 * 256
DEFAULT = (11, 0.01)                                   # frac_bits, min_maf: hpgv_grm_frac_bits(0.01)
EXTREME = (14, 0.5)                                    # only rows with X == Y are used: q = -23170, 0, 23170


def table(class3, frac_bits, min_maf):
    """(used [rows] bool, q [rows, 3] int64) of class counts [rows, >= 3]: numpy f64 in the header's order, zeros where unused"""
    c = np.asarray(class3, np.int64)
    n0, n1, n2 = c[:, 0], c[:, 1], c[:, 2]
    X, Y = 2 * n0 + n1, n1 + 2 * n2
    T = X + Y
    ok = (n0 >= 0) & (n1 >= 0) & (n2 >= 0) & (0 < Y) & (Y < T)
    with np.errstate(all="ignore"):
        Tf = T.astype(np.float64)
        ok &= np.minimum(X, Y).astype(np.float64) / Tf >= np.float64(min_maf)
        p = Y.astype(np.float64) / Tf
        d = np.sqrt(np.float64(2.0) * p * (np.float64(1.0) - p))
        z = (np.arange(3, dtype=np.float64)[None, :] - (np.float64(2.0) * p)[:, None]) / d[:, None]
        r = np.rint(z * np.float64(2.0 ** frac_bits))
        ok &= (np.abs(r) <= MAX_Q).all(axis=1)
    q = np.where(ok[:, None], r, 0.0).astype(np.int64)
    return ok, q


def limbs(q):
    """(hi, lo) int64 of q: lo = (int8)(q & 0xFF), hi = (q - lo) / 256"""
    q = np.asarray(q, np.int64)
    lo = (q & 0xFF).astype(np.uint8).view(np.int8).astype(np.int64).reshape(q.shape)
    return (q - lo) // 256, lo


def tab_records(used, q):
    """the GRM_TAB records of hpgv_grm_table / hpgv_grm_table_dev"""
    hi, lo = limbs(q)
    out = np.zeros(len(q), hpgv.GRM_TAB)
    out["hi"][:, :3], out["lo"][:, :3] = hi, lo
    return out


def z_table(class3, min_maf):
    """the UNQUANTISED z [rows, 3] in long double, for the quantisation bound"""
    c = np.asarray(class3, np.int64)
    X, Y = 2 * c[:, 0] + c[:, 1], c[:, 1] + 2 * c[:, 2]
    f = np.longdouble
    with np.errstate(all="ignore"):
        p = Y.astype(f) / (X + Y).astype(f)
        return (np.arange(3).astype(f)[None, :] - (2 * p)[:, None]) / np.sqrt(2 * p * (1 - p))[:, None]


def golden(codes, frac_bits, min_maf, skip=None):
    """dict: class4 [rows, 4] (zeros for a skipped row), used [rows], q [rows, 3], acc int64 [cols, cols, 2] = {sq, n} for
    i <= j and zeros elsewhere"""
    codes = np.asarray(codes)
    class4 = ig.class_counts(codes, skip)
    used, q = table(class4, frac_bits, min_maf)
    if skip is not None:
        used = used & (np.asarray(skip) == 0)
        q = np.where(used[:, None], q, 0)
    valid, g = classes(codes)
    V = (valid & used[:, None]).astype(np.int64)
    Q = np.take_along_axis(q, g, axis=1) * V
    acc = np.stack([Q.T @ Q, V.T @ V], axis=-1)
    acc[~np.triu(np.ones(acc.shape[:2], bool))] = 0
    return dict(class4=class4, used=used, q=q, acc=acc)


def value(acc, frac_bits):
    """((double)sq * 2^(-2s)) / (double)n of int64 [..., 2]"""
    a = np.asarray(acc, np.int64)
    with np.errstate(all="ignore"):
        return (a[..., 0].astype(np.float64) * np.float64(2.0 ** (-2 * frac_bits))) / a[..., 1].astype(np.float64)


def files(acc, frac_bits, names):
    """the runner's three files as bytes: rows i = 0 .. n - 1, columns j = 0 .. i, the element (i, j) from acc[j, i]"""
    n = len(names)
    val = value(acc, frac_bits).astype(np.float32)
    il = np.tril_indices(n)                                      # row-major: (0, 0), (1, 0), (1, 1), ...
    return {".grm.bin": val.T[il].tobytes(), ".grm.N.bin": acc[..., 1].T[il].astype(np.float32).tobytes(),
            ".grm.id": "".join("%s\t%s\n" % (s, s) for s in names).encode()}


@functools.lru_cache(maxsize=None)
def balanced(rows, cols):
    """codes [rows, cols] where every second row has as many class-0 as class-2 calls (X == Y: used at min_maf 0.5), with
    heterozygotes, "1/2" and missing bytes among them; the other rows are ig.matrix's.  Read-only, shared by the tests"""
    rng = np.random.default_rng(9100 + 1000 * cols + rows)
    codes = ig.matrix(rows, cols).copy()
    for r in range(0, rows, 2):
        k = int(rng.integers(0, cols // 2 + 1))
        miss = int(rng.integers(0, max(cols - 2 * k, 0) // 4 + 1))
        row = np.concatenate([np.full(k, 0x00), rng.choice([0x11, 0x12, 0x21], k), rng.choice([0xFF, 0x0F, 0xF1], miss),
                              rng.choice([0x01, 0x10, 0x02], cols - 2 * k - miss)]).astype(np.uint8)
        codes[r] = rng.permutation(row)
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def golden_of(rows, cols, which):
    """the golden of ig.matrix at DEFAULT (which = 0) or of balanced at EXTREME (which = 1); read-only"""
    out = golden(ig.matrix(rows, cols) if which == 0 else balanced(rows, cols), *(DEFAULT, EXTREME)[which])
    for a in out.values():
        a.setflags(write=False)
    return out


PATTERN = 0x5A5A5A5A5A5A5A5A


def fresh_acc(n_cols):
    """the caller's buffer before the first call: zeros for i <= j, a pattern elsewhere -- which must come back unchanged"""
    buf = np.full((n_cols, n_cols, 2), PATTERN, np.int64)
    buf[np.triu(np.ones((n_cols, n_cols), bool))] = 0
    return buf


def check_acc(got, exp, what=""):
    """the sums where i <= j, the pattern elsewhere"""
    nc = got.shape[0]
    upper = np.triu(np.ones((nc, nc), bool))
    assert (got[~upper] == PATTERN).all(), "%s: an element with i > j was touched" % what
    bad = np.argwhere((got[upper] != np.asarray(exp)[upper]).any(axis=-1))
    assert len(bad) == 0, "%s: sums differ at %s: %s against %s" % (what, np.argwhere(upper)[bad[:4, 0]].tolist(), got[upper][bad[:2, 0]].tolist(),
                                                                  np.asarray(exp)[upper][bad[:2, 0]].tolist())


class DevAcc:
    """a buffer of pair sums on the device for a run of calls"""

    def __init__(self, e, n_cols):
        self.e, self.n_cols = e, n_cols
        self.d = e.alloc(max(n_cols * n_cols * 16, 16))
        e.h2d(self.d, fresh_acc(n_cols))

    def get(self):
        self.e.sync()
        return self.e.d2h(self.d, (self.n_cols, self.n_cols, 2), np.int64)

    def close(self):
        self.e.free(self.d)


def add_dev(e, da, laid, n_cols, frac_bits, min_maf, skip=None):
    """class counts, table and pair sums of a laid-out matrix by the three device calls, into a DevAcc.  Returns what
    hpgv_grm_table_dev left: (table records [rows], skip bytes [rows], used count)"""
    laid = np.ascontiguousarray(laid, np.uint8)
    nv, pitch = laid.shape
    d_gt, d_skip, d_c4, d_tab, d_n = e.alloc(max(laid.nbytes, 16)), e.alloc(max(nv, 16)), e.alloc(nv * 16), e.alloc(nv * 8), e.alloc(16)
    e.h2d(d_gt, laid)
    e.h2d(d_skip, np.zeros(nv, np.uint8) if skip is None else np.asarray(skip, np.uint8))
    e.h2d(d_tab, np.full(nv, 0x77, np.int64))
    e.h2d(d_n, np.full(4, 0x77, np.int32))
    e.ibs_class_counts_dev(d_gt, pitch, nv, n_cols, d_c4, d_skip=d_skip)
    e.grm_table_dev(d_c4, nv, frac_bits, min_maf, d_skip, d_tab, d_n)
    e.grm_pairs_dev(d_gt, pitch, nv, n_cols, d_tab, da.d, d_skip=d_skip)
    e.sync()
    out = e.d2h(d_tab, (nv,), hpgv.GRM_TAB), e.d2h(d_skip, (nv,), np.uint8), int(e.d2h(d_n, (1,), np.int32)[0])
    for b in (d_gt, d_skip, d_c4, d_tab, d_n):
        e.free(b)
    return out


def run_dev(e, laid, n_cols, frac_bits, min_maf, skip=None):
    """one call into a fresh buffer: the whole [n_cols, n_cols, 2] buffer"""
    da = DevAcc(e, n_cols)
    add_dev(e, da, laid, n_cols, frac_bits, min_maf, skip)
    out = da.get()
    da.close()
    return out
