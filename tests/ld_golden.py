"""Goldens of the LD band (include/hpgv.h "LD"), built in numpy from the code matrix: the planes from the byte classes, counts6 from
int64 products of the band, r2 by the header's expression in float64 on the exact integers; and the helpers the tests share."""
import functools

import numpy as np

from helpers import hpgv, random_codes
from model_golden import bits, classes

WIDTHS = [(2, 3), (37, 45), (64, 64), (301, 412)]      # (affected, unaffected): five columns; two ragged k-steps; whole chunks; 12 k-steps, the last ragged
VARIANTS = [1, 2, 17, 65, 150, 300]                    # no pair; one; a ragged wave; a pair across two A tiles; three tiles; five
WINDOWS = [1, 10, 63, 64, 100, 200, 1024]              # the tile edge at 63 / 64; several B groups from 100 on


def r2_of(c6):
    """the header's expression on int64 counts (..., 6): exact differences, then float64 in the stated order; 0 / 0 = NaN"""
    n, sa, sb, saa, sbb, sab = (np.asarray(c6, np.int64)[..., k] for k in range(6))
    cov, va, vb = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
    with np.errstate(invalid="ignore", divide="ignore"):
        return (cov.astype(np.float64) * cov.astype(np.float64)) / (va.astype(np.float64) * vb.astype(np.float64))


def band(codes, window, b_begin=0, chrom=None, pos=None, max_bp=-1, skip=None):
    """(r2 [nv - b_begin, window], counts6 [.., window, 6] int32, in-band mask) of the rows of a code matrix; element [b - b_begin, d - 1]
    is the pair (b - d, b)"""
    nv = len(codes)
    valid, dosage = classes(codes)
    V, G = valid.astype(np.int64), dosage.astype(np.int64)
    Q = G * G
    c6 = np.zeros((nv, window, 6), np.int64)
    inband = np.zeros((nv, window), bool)
    for d in range(1, min(window, nv - 1) + 1):
        a, b = slice(0, nv - d), slice(d, nv)
        for k, (x, y) in enumerate(((V, V), (G, V), (V, G), (Q, V), (V, Q), (G, G))):
            c6[d:, d - 1, k] = (x[a] * y[b]).sum(axis=1)
        ok = np.ones(nv - d, bool)
        if skip is not None:
            s = np.asarray(skip) != 0
            ok &= ~s[a] & ~s[b]
        if chrom is not None:
            ch, po = np.asarray(chrom, np.int64), np.asarray(pos, np.int64)
            ok &= ch[a] == ch[b]
            if max_bp >= 0:
                ok &= np.abs(po[b] - po[a]) <= max_bp
        inband[d:, d - 1] = ok
    c6[~inband] = 0
    r2 = r2_of(c6)
    r2[~inband] = np.nan
    return r2[b_begin:], c6[b_begin:].astype(np.int32), inband[b_begin:]


def lay(codes, n_affected):
    """a code matrix [affected columns | unaffected columns] as the assoc layout holds it: each part padded with 0xFF to whole
    16-byte chunks"""
    nv, ns = codes.shape
    pa, pu = -(-n_affected // 16) * 16, -(-(ns - n_affected) // 16) * 16
    out = np.full((nv, max(pa + pu, 16)), 0xFF, np.uint8)
    out[:, :n_affected] = codes[:, :n_affected]
    out[:, pa:pa + ns - n_affected] = codes[:, n_affected:]
    return out


@functools.lru_cache(maxsize=None)
def matrix(width, nv, quirks=True):
    """random codes [nv, affected + unaffected]; read-only, shared by the tests"""
    rng = np.random.default_rng(9100 + 100 * width[0] + nv)
    codes = random_codes(rng, nv, width[0] + width[1], quirks=quirks, strict=False)
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def golden(width, nv, window):
    out = band(matrix(width, nv), window)
    for a in out:
        a.setflags(write=False)
    return out


def flip(row):
    """g -> 2 - g on the called bytes of a row, missing ones stay missing"""
    valid, dosage = classes(row)
    return np.where(valid, np.array([0x11, 0x01, 0x00], np.uint8)[dosage], 0xFF).astype(np.uint8)


def run_dev(e, laid, window, b_begin=0, chrom=None, pos=None, max_bp=-1, skip=None, counts=True):
    """hpgv_ld_window_dev on a laid-out matrix: (r2, counts6).  The outputs are filled with a pattern first: every element of the
    band is to be written"""
    laid = np.ascontiguousarray(laid, np.uint8)
    nv, pitch = laid.shape
    nb = nv - b_begin
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
    d_r2 = up(np.full((nb, window), 12345.0))
    d_c6 = up(np.full((nb, window, 6), 0x5A5A5A5A, np.int32)) if counts else None
    e.ld_window_dev(d_gt, pitch, nv, window, d_r2, d_c6, b_begin=b_begin, d_chrom=d_chrom, d_pos=d_pos, max_bp=max_bp, d_skip=d_skip)
    e.sync()
    r2 = e.d2h(d_r2, (nb, window), np.float64) if nb else np.zeros((0, window))
    c6 = (e.d2h(d_c6, (nb, window, 6), np.int32) if nb else np.zeros((0, window, 6), np.int32)) if counts else None
    for b in bufs:
        e.free(b)
    return r2, c6


def assert_same(got, exp, what=""):
    """counts6 equal; r2 NaN in the same places and bit for bit equal elsewhere (which NaN is not defined)"""
    (r2, c6), (x2, x6) = got[:2], exp[:2]
    assert r2.shape == x2.shape, what
    if c6 is not None:
        assert np.array_equal(c6, x6), "%s: counts6 differ at %s" % (what, np.argwhere((c6 != x6).any(axis=-1))[:4].tolist())
    nan = np.isnan(x2)
    assert np.array_equal(np.isnan(r2), nan), "%s: NaN pattern differs at %s" % (what, np.argwhere(np.isnan(r2) != nan)[:4].tolist())
    assert np.array_equal(bits(r2)[~nan], bits(x2)[~nan]), "%s: r2 bits differ" % what


def engine():
    return hpgv.Engine(0)
