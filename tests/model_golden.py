"""Goldens of the model tests (include/hpgv.h "model tests"), built in numpy and exact rational arithmetic from the code
matrix: genotype classes, the counts8 record, the five statistics and their p-values, and the cases the GPU tests share."""
import functools
from fractions import Fraction

import numpy as np
import scipy.stats

from helpers import close, hpgv, random_codes

GENO, TREND, ALLELIC, DOM, REC = range(5)
DF = np.array([2, 1, 1, 1, 1])


def strict(codes):
    """the assoc layout's view of a code matrix: a half-called genotype is a missing one"""
    return np.where(((codes >> 4) == 15) | ((codes & 15) == 15), 0xFF, codes).astype(np.uint8)


def classes(codes):
    """(valid, dosage) of a code matrix by the header's class table: missing when either nibble is 0xF, else the number of
    nibbles that are not 0"""
    hi, lo = codes >> 4, codes & 15
    valid = (hi != 15) & (lo != 15)
    dosage = np.where(valid, (hi != 0).astype(np.int64) + (lo != 0), 0)
    return valid, dosage


def counts8(codes, cond):
    """{r0, r1, r2, s0, s1, s2, miss_aff, miss_unaff} per row"""
    valid, dosage = classes(codes)
    out = np.zeros((codes.shape[0], 8), np.int32)
    for g, sel in enumerate((cond == 1, cond == 0)):
        for k in range(3):
            out[:, 3 * g + k] = (valid[:, sel] & (dosage[:, sel] == k)).sum(axis=1)
        out[:, 6 + g] = (~valid[:, sel]).sum(axis=1)
    return out


def trend_exact(N, W1, W2, R, D):
    """N (N D - R W1)^2 / (R (N - R) (N W2 - W1^2)) in rational arithmetic, rounded once; NaN where the denominator is 0"""
    N, W1, W2, R, D = (np.broadcast_arrays(N, W1, W2, R, D))
    out = np.full(N.shape, np.nan)
    flat = out.reshape(-1)
    for i, (n, w1, w2, r, d) in enumerate(zip(*(a.reshape(-1).tolist() for a in (N, W1, W2, R, D)))):
        den = r * (n - r) * (n * w2 - w1 * w1)
        if den:
            a = n * d - r * w1
            flat[i] = float(Fraction(n * a * a, den))
    return out


def pearson(table):
    """explicit Pearson sum of [n, 2, k] tables, NaN where an expected value is 0"""
    t = table.astype(np.float64)
    row, col, n = t.sum(axis=2, keepdims=True), t.sum(axis=1, keepdims=True), t.sum(axis=(1, 2), keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = row * col / n
        x = ((t - e) ** 2 / e).sum(axis=(1, 2))
    x[(e == 0).any(axis=(1, 2)) | np.isnan(e).any(axis=(1, 2))] = np.nan
    return x


def margins(c8):
    c = c8.astype(np.int64)
    r, s = c[:, 0:3], c[:, 3:6]
    n = r + s
    return r, s, n, r.sum(axis=1), n.sum(axis=1), n[:, 1] + 2 * n[:, 2], n[:, 1] + 4 * n[:, 2], r[:, 1] + 2 * r[:, 2]


def statistics(c8):
    """(chisq5, p5) of counts8 rows"""
    r, s, n, R, N, W1, W2, D = margins(c8)
    two = lambda a, b, c, d: pearson(np.stack([np.stack([a, b], axis=1), np.stack([c, d], axis=1)], axis=1))
    x = np.zeros((len(c8), 5))
    x[:, GENO] = pearson(np.stack([r, s], axis=1))
    x[:, TREND] = trend_exact(N, W1, W2, R, D)
    x[:, ALLELIC] = two(2 * r[:, 0] + r[:, 1], r[:, 1] + 2 * r[:, 2], 2 * s[:, 0] + s[:, 1], s[:, 1] + 2 * s[:, 2])
    x[:, DOM] = two(r[:, 1] + r[:, 2], r[:, 0], s[:, 1] + s[:, 2], s[:, 0])
    x[:, REC] = two(r[:, 2], r[:, 0] + r[:, 1], s[:, 2], s[:, 0] + s[:, 1])
    return x, scipy.stats.chi2.sf(x, DF[None, :])


def cross_check(codes, cond, c8, chisq5):
    """the goldens against independent formulations: TREND = N corrcoef(dosage, label)^2 over the genotyped cohort samples;
    the Pearson tests = scipy's chi2_contingency on rows with all margins positive"""
    valid, dosage = classes(codes)
    cohort = cond != 2
    y = (cond == 1).astype(np.float64)
    r, s, n, *_ = margins(c8)
    for v in range(len(codes)):
        sel = valid[v] & cohort
        if not np.isnan(chisq5[v, TREND]):
            rho = np.corrcoef(dosage[v, sel].astype(np.float64), y[sel])[0, 1]
            assert close(sel.sum() * rho * rho, chisq5[v, TREND]), ("trend", v)
        tabs = {GENO: np.stack([r[v], s[v]]),
                ALLELIC: np.array([[2 * r[v, 0] + r[v, 1], r[v, 1] + 2 * r[v, 2]], [2 * s[v, 0] + s[v, 1], s[v, 1] + 2 * s[v, 2]]]),
                DOM: np.array([[r[v, 1] + r[v, 2], r[v, 0]], [s[v, 1] + s[v, 2], s[v, 0]]]),
                REC: np.array([[r[v, 2], r[v, 0] + r[v, 1]], [s[v, 2], s[v, 0] + s[v, 1]]])}
        for t, tab in tabs.items():
            if (tab.sum(axis=0) > 0).all() and (tab.sum(axis=1) > 0).all():
                assert close(scipy.stats.chi2_contingency(tab, correction=False)[0], chisq5[v, t]), (t, v)


@functools.lru_cache(maxsize=None)
def case(width, nv, n_perms, quirks, strict_codes=False, special=()):
    """A cohort of width = (affected, unaffected) columns with HPGV_COND_OTHER columns mixed in, nv rows (row 1 all missing, row 2
    monomorphic) and n_perms label rows (row 0 the observed labelling; nobody and everybody affected among them from 5 rows on).
    special: further special label rows, (row, kind) with kind "observed", "nobody" or "everybody", set after the fixed ones."""
    nA, nU = width
    rng = np.random.default_rng(7000 + 1000 * nA + 10 * nv + n_perms + (1 if quirks else 0))
    nO = max(2, (nA + nU) // 8)
    cond = rng.permutation(np.array([1] * nA + [0] * nU + [2] * nO, np.uint8))
    ns = len(cond)
    codes = random_codes(rng, nv, ns, quirks=quirks, strict=strict_codes)
    if nv >= 3:
        codes[1] = 0xFF
        codes[2] = 0x11
    cohort = cond != 2
    labels = (rng.random((n_perms, ns)) < rng.uniform(0.2, 0.8, size=(n_perms, 1))).astype(np.uint8)
    if n_perms:
        labels[0] = cond == 1
    if n_perms >= 5:
        labels[2], labels[n_perms - 1] = 0, 1
    for row, kind in special:
        labels[row] = {"observed": cond == 1, "nobody": 0, "everybody": 1}[kind]
    labels[:, ~cohort] = rng.integers(0, 2, size=(n_perms, int((~cohort).sum())))      # ignored, whatever they hold
    sc = strict(codes)
    c8 = counts8(sc, cond)
    chisq5, p5 = statistics(c8)
    for a in (cond, codes, labels, c8, chisq5, p5):
        a.setflags(write=False)
    return dict(cond=cond, codes=codes, strict=sc, labels=labels, c8=c8, chisq5=chisq5, p5=p5, nv=nv, n_perms=n_perms, ns=ns, width=width)


def engine(c, device=0, labels=True):
    e = hpgv.Engine(device)
    e.set_cohort(c["cond"])
    if labels and c["n_perms"]:
        e.set_perm_labels(c["labels"])
    return e


def run_dev(e, c, rows=slice(None), perm=False):
    """layout, class scan and statistics (and with perm the trend permutation kernel) on device buffers:
    dict(counts8, chisq5, p5, allele counts and chi-square of the allelic scan on the same laid-out rows[, n_ge, batch_max, sums])"""
    codes = np.ascontiguousarray(c["codes"][rows])
    nv, P, ns = len(codes), c["n_perms"], c["ns"]
    pitch = e.assoc_layout()[2]
    sizes = (nv * ns, nv * pitch, nv * 32, nv * 40, nv * 40, nv * 16, nv * 8, nv * 8, nv * 8, nv * 4, P * 8, nv * P * 8)
    bufs = [e.alloc(max(n, 16)) for n in sizes]
    d_raw, d_lay, d_c8, d_x5, d_p5, d_c4, d_odds, d_chi, d_p, d_nge, d_bmax, d_sums = bufs
    if nv:
        e.h2d(d_raw, codes)
        e.layout(hpgv.LAYOUT_ASSOC, d_raw, ns, nv, d_lay)
        e.assoc_model_scan(d_lay, nv, d_c8)
        e.assoc_model_stats(d_c8, nv, d_x5, d_p5)
        e.assoc_scan(d_lay, nv, d_c4)
        e.assoc_chisq(d_c4, nv, d_odds, d_chi, d_p)
    if perm:
        e.h2d(d_bmax, np.full(P, 7.0))                   # overwritten, not merged into
        if nv:
            e.h2d(d_nge, np.full(nv, 9, np.int32))
        e.assoc_trend_perm_dev(d_lay, nv, d_c8, d_nge, d_bmax, d_sums)
    e.sync()
    get = lambda d, shape, dtype: e.d2h(d, shape, dtype) if nv else np.zeros(shape, dtype)
    out = dict(counts8=get(d_c8, (nv, 8), np.int32), chisq5=get(d_x5, (nv, 5), np.float64), p5=get(d_p5, (nv, 5), np.float64),
               counts4=get(d_c4, (nv, 4), np.int32), chisq=get(d_chi, (nv,), np.float64))
    if perm:
        out.update(n_ge=get(d_nge, (nv,), np.int32), batch_max=e.d2h(d_bmax, (P,), np.float64), sums=get(d_sums, (nv, P, 2), np.int32))
    for b in bufs:
        e.free(b)
    return out


def stats_dev(e, c8):
    """the engine's statistics kernel on [n, 8] class tables: chisq5"""
    c8 = np.ascontiguousarray(c8, np.int32)
    n = len(c8)
    d_c, d_x, d_p = e.alloc(max(n * 32, 16)), e.alloc(max(n * 40, 16)), e.alloc(max(n * 40, 16))
    e.h2d(d_c, c8)
    e.assoc_model_stats(d_c, n, d_x, d_p)
    e.sync()
    x = e.d2h(d_x, (n, 5), np.float64)
    for b in (d_c, d_x, d_p):
        e.free(b)
    return x


def text_of(codes):
    """VCF data lines of a code matrix"""
    a1, a2 = codes >> 4, codes & 15
    names = np.array([str(i) for i in range(15)] + ["."])
    cells = np.char.add(np.char.add(names[a1], "/"), names[a2])
    return "".join("7\t%d\trs%d\tA\tC,G,T\t.\tPASS\t.\tGT\t%s\n" % (100 + v, v, "\t".join(cells[v])) for v in range(codes.shape[0])).encode()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
