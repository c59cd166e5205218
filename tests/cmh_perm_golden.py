"""Goldens of the permutation within strata (include/hpgv.h "Permutation within strata"), independent of the code under test: the
permuted per-stratum tables from numpy products of cmh_golden.planes with `labels & (stratum == k)`; the statistic of a (variant,
permutation) as cmh_golden's exact-rational CHISQ_CMH on those tables.  And the cases the GPU tests share: one base case per
(strata, missing rate) at the largest variant and permutation counts, computed once; a test takes its leading rows and label rows
(a label row does not depend on how many rows there are, a variant's values not on the other variants)."""
import ctypes as C
import functools

import numpy as np

import cmh_golden as cg
from helpers import hpgv

N_COHORT, N_OTHER = 150, 7          # three 64-column k-steps, the last one partial
NV_MAX, P_MAX = 130, 300
STRATA = ("one", "three_interleaved", "five_blocks", "seventy")


def perm_tables(codes, cond, stratum, n_strata, labels, is_x=None):
    """[nv, P, K, 4] int32 {a, b, c, d} of every (variant, permutation, stratum): a, b the plane products with the labelled members
    of the stratum, c, d the rest of the stratum's observed allele counts"""
    c1, c2 = cg.planes(cg.strict(codes), is_x)
    cohort = cond != 2
    out = np.zeros((codes.shape[0], len(labels), n_strata, 4), np.int64)
    for k in range(n_strata):
        member = (cohort & (stratum == k)).astype(np.int64)
        y = labels.astype(np.int64) * member                          # [P, ns]
        a, b = c1 @ y.T, c2 @ y.T
        n1, n0 = c1 @ member, c2 @ member                             # A1_k + U1_k, A2_k + U2_k
        out[:, :, k, 0], out[:, :, k, 1] = a, b
        out[:, :, k, 2], out[:, :, k, 3] = n1[:, None] - a, n0[:, None] - b
    assert out.min() >= 0
    return out.astype(np.int32)


def fit_chisq(tabs):
    """hpgv_cmh_fit's chisq of every [K, 4] table set of tabs [..., K, 4], through the C ABI"""
    tabs = np.ascontiguousarray(tabs, np.int32)
    K = tabs.shape[-2]
    n = int(np.prod(tabs.shape[:-2]))
    out = np.zeros(max(n, 1), hpgv.CMH_RESULT)
    L, t0, o0 = hpgv.load(), tabs.ctypes.data, out.ctypes.data
    for i in range(n):
        assert L.hpgv_cmh_fit(C.c_void_p(t0 + i * K * 16), K, C.c_void_p(o0 + i * 72)) == hpgv.OK
    return out["chisq"][:n].reshape(tabs.shape[:-2]).copy()


def rational_chisq(tab):
    """cmh_golden's exact-rational CHISQ_CMH of one [K, 4] table set"""
    return cg.fit(tab)["chisq"]


def strata_of(kind, rng, cond):
    """stratum per VCF column and K.  Every kind but "one" holds a stratum of a single sample (n < 2 on a chr-X row or where its
    call is missing) and a stratum whose samples are all affected (V_k = 0)"""
    ns = len(cond)
    cohort = np.flatnonzero(cond != 2)
    aff = np.flatnonzero(cond == 1)
    st = np.full(ns, -1, np.int32)
    if kind == "one":
        st[cohort] = 0
        K = 1
    elif kind == "three_interleaved":                                 # 0: mixed, 1: one sample, 2: affected only; four cohort columns in none
        K = 3
        st[cohort] = 0
        st[aff[rng.permutation(len(aff))[:9]]] = 2
        rest = cohort[st[cohort] == 0]
        pick = rest[rng.permutation(len(rest))[:5]]
        st[pick[0]] = 1
        st[pick[1:]] = -1
    elif kind == "five_blocks":                                       # blocks of VCF columns: each stratum in few k-steps of the layout
        K = 5
        edges = [0, 50, 51, 100, 110, 150]                            # 1: one sample; 3: made all-affected below
        for k in range(K):
            st[cohort[edges[k]:edges[k + 1]]] = k
    else:
        K = 70
        st[cohort] = rng.integers(0, K, len(cohort))
        st[cohort[st[cohort] == 9]] = 10
        st[aff[:3]] = 9                                               # 9: affected only
        st[cohort[st[cohort] == 7]] = 8
        st[cohort[3]] = 7                                             # 7: one sample
    st[cond == 2] = rng.integers(-3, K + 5, int((cond == 2).sum()))   # not read, whatever they hold
    return st, K


@functools.lru_cache(maxsize=None)
def base(kind, missing):
    """The base case of (strata kind, missing rate): cohort, codes (row 1 all missing, row 2 monomorphic, chr-X rows), strata,
    P_MAX label rows -- two thirds shuffled within strata, the rest fair coins, which keep no class size -- and the goldens: the
    observed tables, the permuted tables and hpgv_cmh_fit's chisq of both"""
    rng = np.random.default_rng(4100 + 10 * STRATA.index(kind) + (1 if missing else 0))
    cond = rng.permutation(np.array([1] * 70 + [0] * (N_COHORT - 70) + [2] * N_OTHER, np.uint8))
    ns = len(cond)
    codes = np.array([0x00, 0x01, 0x10, 0x11, 0x12], np.uint8)[rng.choice(5, size=(NV_MAX, ns), p=[0.4, 0.2, 0.15, 0.2, 0.05])]
    if missing:
        codes[rng.random(codes.shape) < missing] = 0xFF
    codes[1], codes[2] = 0xFF, 0x00
    is_x = (rng.random(NV_MAX) < 0.25).astype(np.uint8)
    is_x[0], is_x[3], is_x[NV_MAX - 1] = 1, 0, 1
    stratum, K = strata_of(kind, rng, cond)
    if kind == "five_blocks":                                         # stratum 3 all affected: its unaffected columns are relabelled
        cond[(stratum == 3) & (cond == 0)] = 1
    n_within = 2 * P_MAX // 3
    labels = np.concatenate([hpgv.perm_labels_shuffle_within(cond, stratum, n_within, 77),
                             (rng.random((P_MAX - n_within, ns)) < 0.5).astype(np.uint8)])
    labels[0] = cond == 1                                             # row 0: the observed labelling, T_0 == T_obs
    tabs = cg.tables(codes, cond, stratum, K, is_x)
    ptabs = perm_tables(codes, cond, stratum, K, labels, is_x)
    t_obs, t_perm = fit_chisq(tabs), fit_chisq(ptabs)
    c = dict(kind=kind, cond=cond, codes=codes, is_x=is_x, stratum=stratum, K=K, ns=ns, labels=labels, tables=tabs, perm_tables=ptabs,
             t_obs=t_obs, t_perm=t_perm)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def expected(c, nv, P, rows=slice(None)):
    """(n_ge, batch_max) the definition gives for the first nv variants (of them, `rows`) and the first P label rows"""
    t, o = c["t_perm"][:nv, :P][rows], c["t_obs"][:nv][rows]
    with np.errstate(invalid="ignore"):
        n_ge = (t >= o[:, None]).sum(axis=1).astype(np.int32)
    bmax = np.where(np.isnan(t), 0.0, t).max(axis=0) if t.shape[0] else np.zeros(P, np.float64)      # 0: nothing entered
    return n_ge, bmax


def engine(c, P, device=0):
    e = hpgv.Engine(device)
    e.set_cohort(c["cond"])
    e.set_strata(c["stratum"], c["K"])
    e.set_perm_labels(c["labels"][:P])
    return e


def run_dev(e, c, nv, P, rows=slice(None), want_chisq=True):
    """layout, hpgv_assoc_cmh_dev and hpgv_assoc_cmh_perm_dev on device buffers: (records, n_ge, batch_max, T [n, P] or None)"""
    codes, is_x = np.ascontiguousarray(c["codes"][:nv][rows]), np.ascontiguousarray(c["is_x"][:nv][rows])
    n, K, ns = len(codes), c["K"], c["ns"]
    pitch = e.assoc_layout()[2]
    bufs = [e.alloc(max(b, 16)) for b in (n * ns, n * pitch, n, n * 72, n * K * 16, n * 4, P * 8, n * P * 8)]
    d_raw, d_lay, d_x, d_out, d_tab, d_nge, d_bmax, d_t = bufs
    if n:
        e.h2d(d_raw, codes)
        e.h2d(d_x, is_x)
        e.layout(hpgv.LAYOUT_ASSOC, d_raw, ns, n, d_lay)
    e.assoc_cmh_dev(d_lay, n, d_out, d_tab, d_x)
    e.assoc_cmh_perm_dev(d_lay, n, d_tab, d_nge, d_bmax, d_t if want_chisq else None, d_x)
    e.sync()
    out = e.d2h(d_out, (n,), hpgv.CMH_RESULT) if n else np.zeros(0, hpgv.CMH_RESULT)
    n_ge = e.d2h(d_nge, (n,), np.int32) if n else np.zeros(0, np.int32)
    bmax = e.d2h(d_bmax, (P,), np.float64)
    t = (e.d2h(d_t, (n, P), np.float64) if n else np.zeros((0, P))) if want_chisq else None
    for b in bufs:
        e.free(b)
    return out, n_ge, bmax, t
