"""Goldens of allele scoring (include/hpgv.h "Score"), built in numpy from the code matrix: the rows' integers in the header's
operation order with np.ldexp and np.rint, the column sums from int64 products over the used rows, the values, the text of the
runner's .profile; and the helpers the tests share."""
import numpy as np

import ibs_golden as ig
from helpers import hpgv
from model_golden import classes

SKIP, FLIP = 1, 2
MAX_Q = 2 ** 28
PATTERN = 0x5A5A5A5A5A5A5A5A


def row_terms(class3, w, s, flags, impute):
    """(used [rows] bool, qg, qm, c int64 [rows, n_scores]) of class counts [rows, >= 3], weights [rows, n_scores], frac_bits
    [n_scores] and flag bytes [rows]: numpy f64 in the header's order, zeros where unused"""
    c3 = np.asarray(class3, np.int64)
    w = np.asarray(w, np.float64).reshape(len(c3), -1)
    s = np.asarray(s, np.int32).reshape(1, -1)
    fl = np.asarray(flags, np.int64).reshape(-1)
    n0, n1, n2 = c3[:, 0], c3[:, 1], c3[:, 2]
    T = 2 * (n0 + n1 + n2)
    flip = (fl & FLIP) != 0
    with np.errstate(all="ignore"):
        p = ((n1 + 2 * n2).astype(np.float64) / T.astype(np.float64))[:, None]
        q = np.rint(np.ldexp(w, s))
        used = ((fl & SKIP) == 0) & (n0 >= 0) & (n1 >= 0) & (n2 >= 0) & (T > 0) & np.isfinite(w).all(axis=1) & (np.abs(q) <= MAX_Q).all(axis=1)
        q = np.where(used[:, None], q, 0.0).astype(np.int64)
        wz = np.where(used[:, None], w, 0.0)
        pz = np.where(used[:, None], p, 0.0)
        imp = np.rint(np.ldexp(wz * (np.float64(2.0) * pz), s)).astype(np.int64)
        imp_f = np.rint(np.ldexp(wz * (np.float64(2.0) * (np.float64(1.0) - pz)), s)).astype(np.int64)
    f = flip[:, None]
    qg = np.where(f, -q, q)
    c = np.where(f, 2 * q, 0)
    qm = np.where(f, (imp_f if impute else 0) - 2 * q, imp if impute else 0)
    z = ~used[:, None]
    return used, np.where(z, 0, qg), np.where(z, 0, qm), np.where(z, 0, c)


def limbs(v):
    """int64 [..., 4]: the balanced limbs of v, low first"""
    v = np.asarray(v, np.int64).copy()
    out = np.zeros(v.shape + (4,), np.int64)
    for i in range(3):
        b = (v & 0xFF).astype(np.uint8).view(np.int8).astype(np.int64).reshape(v.shape)
        out[..., i] = b
        v = (v - b) // 256
    out[..., 3] = v
    return out


def tab_planes(qg, qm, tab_pitch=None):
    """the limb-plane-major table of hpgv_score_table_dev: int8 [n_scores * 8, tab_pitch], zeros past the rows"""
    rows, ns = qg.shape
    tab_pitch = (rows + 63) // 64 * 64 if tab_pitch is None else tab_pitch
    out = np.zeros((ns, 8, tab_pitch), np.int8)
    out[:, :4, :rows] = limbs(qg).transpose(1, 2, 0)
    out[:, 4:, :rows] = limbs(qm).transpose(1, 2, 0)
    return out.reshape(ns * 8, tab_pitch)


def golden(codes, w, s, flags, impute, skip=None):
    """dict: class4 [rows, 4] (zeros for a skipped row), used [rows], qg / qm / c [rows, n_scores], acc int64 [n_scores + 2, cols]
    = the sums, n_called, n_alt, and const int64 [n_scores + 1] = const_k, n_used"""
    codes = np.asarray(codes)
    fl = np.asarray(flags, np.uint8).reshape(-1)
    out = (fl & SKIP) != 0
    if skip is not None:
        out = out | (np.asarray(skip) != 0)
    class4 = ig.class_counts(codes, out.astype(np.uint8))
    used, qg, qm, c = row_terms(class4, w, s, np.where(out, fl | SKIP, fl), impute)
    valid, g = classes(codes)
    G = (g * valid * used[:, None]).astype(np.int64)
    V = (valid & used[:, None]).astype(np.int64)
    M = (~valid & used[:, None]).astype(np.int64)
    acc = np.concatenate([qg.T @ G + qm.T @ M, V.sum(axis=0)[None, :], G.sum(axis=0)[None, :]], axis=0)
    const = np.concatenate([c.sum(axis=0), [used.sum()]]).astype(np.int64)
    return dict(class4=class4, used=used, qg=qg, qm=qm, c=c, acc=acc, const=const)


def value(acc, const, s):
    """value_k[j] = ldexp((double)(sum + const), -s) of acc [n_scores + 2, cols]: float64 [n_scores, cols]"""
    ns = len(const) - 1
    return np.ldexp((acc[:ns] + np.asarray(const)[:ns, None]).astype(np.float64), -np.asarray(s, np.int32).reshape(-1, 1))


def average(acc, const, s, impute):
    """(avg [n_scores, cols], cnt [cols]): value / (2.0 * n), n = n_used with imputation and n_called[j] without"""
    ns = len(const) - 1
    n = np.full(acc.shape[1], const[ns], np.int64) if impute else acc[ns]
    with np.errstate(all="ignore"):
        return value(acc, const, s) / (np.float64(2.0) * n.astype(np.float64)), 2 * n


def profile_text(names, score_names, acc, const, s, impute):
    """the runner's .profile"""
    val = value(acc, const, s)
    avg, cnt = average(acc, const, s, impute)
    ns = len(score_names)
    lines = ["#FID\tIID\tCNT\tCNT2" + "".join("\t%s_SUM\t%s_AVG" % (n, n) for n in score_names)]
    for j, name in enumerate(names):
        lines.append("%s\t%s\t%d\t%d" % (name, name, cnt[j], acc[ns + 1, j]) + "".join("\t%.8g\t%.8g" % (val[k, j], avg[k, j]) for k in range(ns)))
    return "\n".join(lines) + "\n"


def random_inputs(rows, n_scores, seed, p_flip=1 / 3, p_skip=0.05):
    """(w [rows, n_scores], s [n_scores], flags [rows]): weights of mixed magnitudes per column, frac_bits by hpgv_score_frac_bits"""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((rows, n_scores)) * (10.0 ** rng.integers(-3, 4, n_scores))[None, :]
    s = np.array([hpgv.score_frac_bits(np.abs(w[:, k]).max()) for k in range(n_scores)], np.int32)
    flags = (np.where(rng.random(rows) < p_flip, FLIP, 0) | np.where(rng.random(rows) < p_skip, SKIP, 0)).astype(np.uint8)
    if rows >= 15:                                               # at least one of each, whatever the draw
        flags[rows // 2] = FLIP
        if p_skip > 0:
            flags[rows // 3] = SKIP
    return w, s, flags


def acc_pitch_of(n_cols):
    return n_cols + 3


def fresh_acc(n_scores, n_cols):
    """the caller's buffer before the first call: zeros below n_cols, a pattern in the columns past them -- which must come back"""
    buf = np.full((n_scores + 2, acc_pitch_of(n_cols)), PATTERN, np.int64)
    buf[:, :n_cols] = 0
    return buf


def check_acc(got, exp, what=""):
    """(acc, const) against the golden's, array_equal; the pattern past n_cols"""
    acc, const = got
    nc = np.asarray(exp["acc"]).shape[1]
    assert (acc[:, nc:] == PATTERN).all(), "%s: an element past n_cols was touched" % what
    bad = np.argwhere(acc[:, :nc] != exp["acc"])
    assert len(bad) == 0, "%s: sums differ at (plane, column) %s: %s against %s" % (
        what, bad[:6].tolist(), acc[:, :nc][tuple(bad[:6].T)].tolist(), np.asarray(exp["acc"])[tuple(bad[:6].T)].tolist())
    assert np.array_equal(acc[:, :nc], exp["acc"])
    assert np.array_equal(const, exp["const"]), "%s: const / n_used %s against %s" % (what, const.tolist(), np.asarray(exp["const"]).tolist())


class DevAcc:
    """the sums and the constants of a run of calls on the device"""

    def __init__(self, e, n_scores, n_cols):
        self.e, self.n_scores, self.n_cols, self.acc_pitch = e, n_scores, n_cols, acc_pitch_of(n_cols)
        self.d = e.alloc((n_scores + 2) * self.acc_pitch * 8)
        self.d_const = e.alloc((n_scores + 1) * 8)
        e.h2d(self.d, fresh_acc(n_scores, n_cols))
        e.h2d(self.d_const, np.zeros(n_scores + 1, np.int64))

    def get(self):
        self.e.sync()
        return self.e.d2h(self.d, (self.n_scores + 2, self.acc_pitch), np.int64), self.e.d2h(self.d_const, (self.n_scores + 1,), np.int64)

    def close(self):
        self.e.free(self.d)
        self.e.free(self.d_const)


def queue_dev(e, da, laid, n_cols, w, s, flags, impute, skip=None, stream=None, tab_pitch=None):
    """class counts, table and column sums of a laid-out matrix by the three device calls on `stream`, into a DevAcc, not waited
    for: finish_dev of what comes back waits and frees"""
    laid = np.ascontiguousarray(laid, np.uint8)
    nv, pitch = laid.shape
    w = np.ascontiguousarray(w, np.float64).reshape(nv, -1)
    ns = w.shape[1]
    tab_pitch = (nv + 63) // 64 * 64 if tab_pitch is None else tab_pitch
    bufs = d_gt, d_skip, d_c4, d_w, d_fl, d_tab = (e.alloc(max(laid.nbytes, 16)), e.alloc(max(nv, 16)), e.alloc(max(nv * 16, 16)), e.alloc(max(w.nbytes, 16)),
                                                   e.alloc(max(nv, 16)), e.alloc(max(ns * 8 * tab_pitch, 16)))
    e.h2d(d_gt, laid)
    e.h2d(d_skip, np.zeros(nv, np.uint8) if skip is None else np.asarray(skip, np.uint8))
    e.h2d(d_w, w)
    e.h2d(d_fl, np.asarray(flags, np.uint8))
    e.h2d(d_tab, np.full(ns * 8 * tab_pitch, 0x77, np.int8))
    e.sync()
    e.ibs_class_counts_dev(d_gt, pitch, nv, n_cols, d_c4, d_skip=d_skip, stream=stream)
    e.score_table_dev(d_c4, nv, d_w, d_fl, s, impute, d_skip, d_tab, tab_pitch, da.d_const, stream=stream)
    e.score_cols_dev(d_gt, pitch, nv, n_cols, d_tab, tab_pitch, ns, da.d, da.acc_pitch, d_skip=d_skip, stream=stream)
    return dict(bufs=bufs, stream=stream, tab=(d_tab, (ns * 8, tab_pitch)), skip=(d_skip, (nv,)))


def finish_dev(e, q):
    """what hpgv_score_table_dev left: (planes int8 [n_scores * 8, tab_pitch], skip bytes [rows])"""
    if q["stream"] is not None:
        e.sync(q["stream"])
    e.sync()
    out = e.d2h(q["tab"][0], q["tab"][1], np.int8), e.d2h(q["skip"][0], q["skip"][1], np.uint8)
    for b in q["bufs"]:
        e.free(b)
    return out


def add_dev(e, da, laid, n_cols, w, s, flags, impute, skip=None, stream=None, tab_pitch=None):
    return finish_dev(e, queue_dev(e, da, laid, n_cols, w, s, flags, impute, skip, stream, tab_pitch))


def run_dev(e, laid, n_cols, w, s, flags, impute, skip=None):
    """one call into fresh buffers: (acc [n_scores + 2, acc_pitch], const [n_scores + 1])"""
    da = DevAcc(e, np.asarray(w).reshape(len(laid), -1).shape[1], n_cols)
    add_dev(e, da, laid, n_cols, w, s, flags, impute, skip)
    out = da.get()
    da.close()
    return out
