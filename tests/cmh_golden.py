"""Goldens of the stratified association (include/hpgv.h "stratified association"), independent of the code under test: the
per-stratum allele tables from numpy products of the planes (c1, c2) with 0 / 1 stratum indicators; CHISQ_CMH and OR_MH as exact
rationals converted once; the Robins-Breslow-Greenland SE from exact rational sums; Breslow-Day in 60-digit decimal arithmetic
(the textbook root formula -- at 60 digits its cancellation does not matter -- and the root chosen by its interval); the tails by
math.erfc / math.exp closed forms, cross-checked against scipy where it is installed.  And the cases the tests share."""
import functools
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

from helpers import hpgv, random_codes

getcontext().prec = 60
Z95 = 1.959963984540054
NAN = math.nan


# ---- tables ---------------------------------------------------------------------------------------------------------------

def strict(codes):
    """the assoc layout's view of a code matrix: a half-called genotype is a missing one"""
    return np.where(((codes >> 4) == 15) | ((codes & 15) == 15), 0xFF, codes).astype(np.uint8)


def planes(codes, is_x=None):
    """(c1, c2) per sample of a strict code matrix, int64 [nv, ns]: reference alleles and alternate alleles; rows with is_x by the
    chr-X rule (1 for byte 0x00; 1 for a byte whose nibbles are both alternate alleles)"""
    hi, lo = (codes >> 4).astype(np.int64), (codes & 15).astype(np.int64)
    alt_hi, alt_lo = (hi != 0) & (hi != 15), (lo != 0) & (lo != 15)
    c1 = (hi == 0).astype(np.int64) + (lo == 0)
    c2 = alt_hi.astype(np.int64) + alt_lo
    if is_x is not None:
        x = np.asarray(is_x).astype(bool)[:, None]
        c1 = np.where(x, (codes == 0).astype(np.int64), c1)
        c2 = np.where(x, (alt_hi & alt_lo).astype(np.int64), c2)
    return c1, c2


def tables(codes, cond, stratum, n_strata, is_x=None):
    """[nv, K, 4] int32 {A1, A2, U1, U2} per stratum: c1 @ indicator.T and c2 @ indicator.T"""
    c1, c2 = planes(strict(codes), is_x)
    ind = np.zeros((2 * n_strata, len(cond)), np.int64)
    for k in range(n_strata):
        ind[2 * k] = (stratum == k) & (cond == 1)
        ind[2 * k + 1] = (stratum == k) & (cond == 0)
    t1, t2 = c1 @ ind.T, c2 @ ind.T
    out = np.zeros((codes.shape[0], n_strata, 4), np.int32)
    out[:, :, 0], out[:, :, 1], out[:, :, 2], out[:, :, 3] = t1[:, 0::2], t2[:, 0::2], t1[:, 1::2], t2[:, 1::2]
    return out


# ---- tails ----------------------------------------------------------------------------------------------------------------

def tail1(x):
    """the project's 1-df tail: 1 - P(x) evaluated in f64 as the reference does (1 - gsl_cdf_chisq_P(x, 1)), on Python's libm"""
    if x != x:
        return NAN
    if x <= 0.0:
        return 1.0
    y = x / 2.0
    P = 1.0 - math.erfc(math.sqrt(y)) if y > 0.5 else math.erf(math.sqrt(y))
    return 1.0 - P


def tail(x, df):
    """the upper chi-square tail for an integer df by the finite closed forms, every term written out"""
    if df == 1:
        return tail1(x)
    if x != x or df < 1:
        return NAN
    if x <= 0.0:
        return 1.0
    h = x / 2.0
    if df % 2 == 0:
        p = math.exp(-h) * math.fsum(h ** i / math.factorial(i) for i in range(df // 2))
    else:
        odd = lambda i: math.prod(range(1, 2 * i, 2))                 # 1 . 3 ... (2i - 1)
        p = math.erfc(math.sqrt(h)) + math.sqrt(2.0 * x / math.pi) * math.exp(-h) * math.fsum(x ** (i - 1) / odd(i) for i in range(1, (df - 1) // 2 + 1))
    return min(p, 1.0)


# ---- statistics -----------------------------------------------------------------------------------------------------------

def fitted(psi, m1, m0, n1):
    """Breslow-Day's fitted count (Decimal) for the odds ratio psi (Decimal): the root of the quadratic inside
    [max(0, n1 - m0), min(m1, n1)], or None when no root lies there"""
    qa, qb, qc = 1 - psi, (m0 - n1) + psi * (m1 + n1), -psi * m1 * n1
    lo, hi = max(0, n1 - m0), min(m1, n1)
    if qa == 0:
        roots = [-qc / qb]
    else:
        d = (qb * qb - 4 * qa * qc).sqrt()
        roots = [(-qb + d) / (2 * qa), (-qb - d) / (2 * qa)]
    inside = [r for r in roots if lo <= r <= hi]
    assert len(inside) <= 1 or abs(inside[0] - inside[1]) < Decimal(10) ** -40
    return inside[0] if inside else None


def fit(tab):
    """the record of one variant from its [K, 4] tables, as a dict with the fields of hpgv_cmh_result (and "fitted": the entered
    strata's (k, A_k))"""
    T = [tuple(int(x) for x in row) for row in np.asarray(tab).reshape(-1, 4)]
    part = [(a, b, c, d) for a, b, c, d in T if a + b + c + d >= 2]
    sa = sum(a for a, b, c, d in part)
    sE = sum((Fraction((a + b) * (a + c), a + b + c + d) for a, b, c, d in part), Fraction(0))
    sV = sum((Fraction((a + b) * (c + d) * (a + c) * (b + d), (a + b + c + d) ** 2 * (a + b + c + d - 1)) for a, b, c, d in part), Fraction(0))
    r = dict(n_strata_cmh=len(part), chisq=float((sa - sE) ** 2 / sV) if sV > 0 else NAN)
    r["p"] = tail1(r["chisq"])
    F = lambda num, n: Fraction(num, n)
    sR = sum((F(a * d, a + b + c + d) for a, b, c, d in part), Fraction(0))
    sS = sum((F(b * c, a + b + c + d) for a, b, c, d in part), Fraction(0))
    has_or = sR > 0 and sS > 0
    if has_or:
        psi = sR / sS
        sPR = sum((F(a + d, a + b + c + d) * F(a * d, a + b + c + d) for a, b, c, d in part), Fraction(0))
        sQS = sum((F(b + c, a + b + c + d) * F(b * c, a + b + c + d) for a, b, c, d in part), Fraction(0))
        sX = sum((F(a + d, a + b + c + d) * F(b * c, a + b + c + d) + F(b + c, a + b + c + d) * F(a * d, a + b + c + d) for a, b, c, d in part), Fraction(0))
        var = sPR / (2 * sR * sR) + sX / (2 * sR * sS) + sQS / (2 * sS * sS)
        se = math.sqrt(float(var))
        l = math.log(float(psi))
        r.update(or_mh=float(psi), se=se, l95=math.exp(l - Z95 * se), u95=math.exp(l + Z95 * se))
    else:
        r.update(or_mh=NAN, se=NAN, l95=NAN, u95=NAN)
    entered = [(k, t) for k, t in enumerate(T) if t[0] + t[1] > 0 and t[2] + t[3] > 0 and t[0] + t[2] > 0 and t[1] + t[3] > 0]
    r["n_strata_bd"] = len(entered)
    r["chisq_bd"], r["p_bd"], r["fitted"] = NAN, NAN, []
    if has_or and len(entered) >= 2:
        psi_d = Decimal(psi.numerator) / Decimal(psi.denominator)
        x2, ok = Decimal(0), True
        for k, (a, b, c, d) in entered:
            m1, m0, n1 = a + b, c + d, a + c
            A = fitted(psi_d, m1, m0, n1)
            cells = None if A is None else (A, m1 - A, n1 - A, m0 - n1 + A)
            if cells is None or min(cells) <= 0:
                ok = False
                break
            W = 1 / sum(1 / x for x in cells)
            x2 += (a - A) ** 2 / W
            r["fitted"].append((k, A))
        if ok:
            r["chisq_bd"] = float(x2)
            r["p_bd"] = tail(r["chisq_bd"], len(entered) - 1)
    return r


FIELDS = ("chisq", "p", "or_mh", "se", "l95", "u95", "chisq_bd", "p_bd")


def fit_all(tabs):
    """fit of every variant of [nv, K, 4] tables: a dict of arrays"""
    recs = [fit(t) for t in tabs]
    out = {k: np.array([r[k] for r in recs], np.float64) for k in FIELDS}
    out.update({k: np.array([r[k] for r in recs], np.int32) for k in ("n_strata_cmh", "n_strata_bd")})
    return out


def common_or_tables(rng, K, ratio=2):
    """K strata with one common integer odds ratio: a d == ratio b c in each, all cells positive"""
    out = np.zeros((K, 4), np.int32)
    for k in range(K):
        b, c = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        d = int(rng.integers(1, 7))
        m = b * c * ratio                                             # a d = m, d | m
        while m % d:
            d -= 1
        out[k] = (m // d, b, c, d)
    return out


def format_f6(x):
    return "nan" if x != x else "%6f" % x


def format_line(chrom, pos, vid, ref, alt, r):
    """the runner's line for a result r: a dict or record with the fields of hpgv_cmh_result"""
    return "\t".join([chrom, str(pos), vid, ref, alt, str(int(r["n_strata_cmh"]))] + [format_f6(float(r[k])) for k in FIELDS])


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(width, nv, K, quirks=True, everyone=False):
    """A cohort of width = (affected, unaffected) columns with HPGV_COND_OTHER columns mixed in, nv rows of quirk genotype codes
    (row 1 all missing, row 2 monomorphic, a fifth of the rows on chr X) and a stratum in 0 .. K - 1 per sample -- one in twelve
    in no stratum (-1) unless `everyone`; what the HPGV_COND_OTHER columns hold is arbitrary.  With the oracle's tables and records."""
    nA, nU = width
    rng = np.random.default_rng(9000 + 1000 * nA + 10 * nv + K + (1 if quirks else 0) + (500 if everyone else 0))
    nO = max(2, (nA + nU) // 8)
    cond = rng.permutation(np.array([1] * nA + [0] * nU + [2] * nO, np.uint8))
    ns = len(cond)
    codes = random_codes(rng, nv, ns, quirks=quirks, strict=False)
    is_x = (rng.random(nv) < 0.2).astype(np.uint8)
    if nv >= 3:
        codes[1] = 0xFF
        codes[2] = 0x00
        is_x[0], is_x[nv - 1] = 1, 0
    stratum = rng.integers(0, K, ns).astype(np.int32)
    if not everyone:
        stratum[rng.random(ns) < 1 / 12] = -1
    stratum[cond == 2] = rng.integers(-3, K + 5, int((cond == 2).sum()))      # not read, whatever they hold
    tabs = tables(codes, cond, stratum, K, is_x)
    ref = fit_all(tabs)
    for a in (cond, codes, is_x, stratum, tabs) + tuple(ref.values()):
        a.setflags(write=False)
    return dict(cond=cond, codes=codes, is_x=is_x, stratum=stratum, K=K, tables=tabs, ref=ref, nv=nv, ns=ns, width=width)


def engine(c, device=0):
    e = hpgv.Engine(device)
    e.set_cohort(c["cond"])
    e.set_strata(c["stratum"], c["K"])
    return e


def run_dev(e, c, rows=slice(None), own_tables=True):
    """layout and hpgv_assoc_cmh_dev on device buffers: (records, tables [nv, K, 4] or None when the context's scratch holds them)"""
    codes, is_x = np.ascontiguousarray(c["codes"][rows]), np.ascontiguousarray(c["is_x"][rows])
    nv, K, ns = len(codes), c["K"], c["ns"]
    pitch = e.assoc_layout()[2]
    bufs = [e.alloc(max(n, 16)) for n in (nv * ns, nv * pitch, nv, nv * 72, nv * K * 16)]
    d_raw, d_lay, d_x, d_out, d_tab = bufs
    if nv:
        e.h2d(d_raw, codes)
        e.h2d(d_x, is_x)
        e.layout(hpgv.LAYOUT_ASSOC, d_raw, ns, nv, d_lay)
    e.assoc_cmh_dev(d_lay, nv, d_out, d_tab if own_tables else None, d_x)
    e.sync()
    out = e.d2h(d_out, (nv,), hpgv.CMH_RESULT) if nv else np.zeros(0, hpgv.CMH_RESULT)
    tab = (e.d2h(d_tab, (nv, K, 4), np.int32) if nv else np.zeros((0, K, 4), np.int32)) if own_tables else None
    for b in bufs:
        e.free(b)
    return out, tab


def text_of(codes, chrom="7"):
    """VCF data lines of a code matrix"""
    a1, a2 = codes >> 4, codes & 15
    names = np.array([str(i) for i in range(15)] + ["."])
    cells = np.char.add(np.char.add(names[a1], "/"), names[a2])
    return "".join("%s\t%d\trs%d\tA\tC,G,T\t.\tPASS\t.\tGT\t%s\n" % (chrom, 100 + v, v, "\t".join(cells[v])) for v in range(codes.shape[0])).encode()
