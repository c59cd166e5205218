"""Label permutation of the association test (k_assoc_perm, csrc/hpgv_assoc_perm_kernels.h): the permuted allele counts off the
matrix cores bit-exact against the oracle's counts under every relabelling, n_ge and batch_max exact against the engine's own
chi-square kernel run on the oracle's permuted counts (and within TOL of the oracle's statistics), the host and text entry
points, splitting, a group context and the label state."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import TOL, assert_close, hpgv, random_codes
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

WIDTHS = [(2, 3), (37, 45), (64, 64), (301, 412)]      # (affected, unaffected): 5 columns; two ragged k-steps; whole chunks; 12 k-steps, the last ragged
VARIANTS = [1, 17, 150]                                 # one row; a ragged 16-row tile; three workgroups, the last ragged
PERMS = [1, 5, 33, 100]                                 # below one 16-column tile; ragged tiles


def _strict(codes):
    """the assoc layout's view of a code matrix: a half-called genotype is a missing one"""
    return np.where(((codes >> 4) == 15) | ((codes & 15) == 15), 0xFF, codes).astype(np.uint8)


def _special_rows(labels, special, observed):
    """further special label rows, (row, kind) with kind "observed", "nobody" or "everybody": set after the fixed ones"""
    for row, kind in special:
        labels[row] = {"observed": observed, "nobody": 0, "everybody": 1}[kind]


@functools.lru_cache(maxsize=None)
def _case(width, nv, n_perms, strict, special=()):
    nA, nU = width
    rng = np.random.default_rng(1000 * nA + 10 * nv + n_perms + (1 if strict else 0))
    nO = max(2, (nA + nU) // 8)
    cond = rng.permutation(np.array([1] * nA + [0] * nU + [2] * nO, np.uint8))
    ns = len(cond)
    codes = random_codes(rng, nv, ns, quirks=True, strict=strict)
    is_x = (rng.random(nv) < 0.2).astype(np.uint8)
    if nv >= 3:
        codes[1] = 0xFF                                  # all missing: T_obs NaN
        codes[2] = 0x00                                  # monomorphic: T_obs NaN
        is_x[0], is_x[nv - 1] = 1, 0
    cohort = cond != 2
    labels = (rng.random((n_perms, ns)) < rng.uniform(0.2, 0.8, size=(n_perms, 1))).astype(np.uint8)
    labels[0] = cond == 1                                # the observed labelling
    if n_perms >= 5:
        labels[2], labels[n_perms - 1] = 0, 1            # nobody affected; everybody affected
    _special_rows(labels, special, cond == 1)
    labels[:, ~cohort] = rng.integers(0, 2, size=(n_perms, int((~cohort).sum())))      # ignored, whatever they hold
    sc = _strict(codes)
    obs = np.stack(orc.assoc_counts(sc, cond, is_x), axis=1)                            # [nv, 4]
    perm = np.zeros((nv, n_perms, 4), np.int32)
    for p in range(n_perms):
        cond_p = cond.copy()
        cond_p[cohort] = labels[p][cohort]
        perm[:, p, :] = np.stack(orc.assoc_counts(sc, cond_p, is_x), axis=1)
    for a in (cond, codes, is_x, labels, obs, perm):
        a.setflags(write=False)
    return dict(cond=cond, codes=codes, is_x=is_x, labels=labels, obs=obs, perm=perm, nv=nv, n_perms=n_perms, ns=ns)


def _engine(c, device=0):
    e = hpgv.Engine(device)
    e.set_cohort(c["cond"])
    e.set_perm_labels(c["labels"])
    return e


def _run_dev(e, c, rows=slice(None)):
    """layout, scan and the permutation kernel on device buffers: (counts, n_ge, batch_max, perm_counts)"""
    codes, is_x = np.ascontiguousarray(c["codes"][rows]), np.ascontiguousarray(c["is_x"][rows])
    nv, P, ns = len(codes), c["n_perms"], c["ns"]
    pitch = e.assoc_layout()[2]
    bufs = [e.alloc(max(n, 16)) for n in (nv * ns, nv * pitch, nv * 16, nv * 4, P * 8, nv * P * 8, nv)]
    d_raw, d_lay, d_counts, d_nge, d_bmax, d_pc, d_x = bufs
    e.h2d(d_bmax, np.full(P, 7.0))                       # overwritten, not merged into
    if nv:
        e.h2d(d_raw, codes)
        e.h2d(d_x, is_x)
        e.h2d(d_nge, np.full(nv, 9, np.int32))
        e.layout(hpgv.LAYOUT_ASSOC, d_raw, ns, nv, d_lay)
        e.assoc_scan(d_lay, nv, d_counts, d_x)
    e.assoc_perm_dev(d_lay, nv, d_counts, d_nge, d_bmax, d_pc, d_x)
    e.sync()
    get = lambda d, shape, dtype: e.d2h(d, shape, dtype) if nv else np.zeros(shape, dtype)
    out = (get(d_counts, (nv, 4), np.int32), get(d_nge, (nv,), np.int32), e.d2h(d_bmax, (P,), np.float64),
           get(d_pc, (nv, P, 2), np.int32))
    for b in bufs:
        e.free(b)
    return out


def _chisq_dev(e, counts):
    """the engine's chi-square kernel on a [n, 4] table of counts"""
    counts = np.ascontiguousarray(counts, np.int32)
    n = len(counts)
    d_c, d_o, d_x, d_p = e.alloc(n * 16), e.alloc(n * 8), e.alloc(n * 8), e.alloc(n * 8)
    e.h2d(d_c, counts)
    e.assoc_chisq(d_c, n, d_o, d_x, d_p)
    e.sync()
    chi = e.d2h(d_x, (n,), np.float64)
    for b in (d_c, d_o, d_x, d_p):
        e.free(b)
    return chi


def _expected(chi, t_obs):
    """n_ge and batch_max of a [nv, P] statistic matrix by the NaN rules"""
    with np.errstate(invalid="ignore"):
        n_ge = (chi >= t_obs[:, None]).sum(axis=1).astype(np.int32)
    bmax = np.fmax.reduce(chi, axis=0, initial=0.0) if chi.shape[0] else np.zeros(chi.shape[1])
    return n_ge, bmax


@functools.lru_cache(maxsize=None)
def _reference(width, nv, n_perms, strict, special=()):
    """(n_ge, batch_max, t_obs) of a case from the engine's chi-square kernel on the ORACLE's permuted counts"""
    c = _case(width, nv, n_perms, strict, special)
    e = hpgv.Engine(0)
    chi = _chisq_dev(e, c["perm"].reshape(-1, 4)).reshape(nv, n_perms)
    t_obs = _chisq_dev(e, c["obs"])
    e.close()
    return _expected(chi, t_obs) + (t_obs,)


CASES = [(w, nv, P, (i + j + k) % 2 == 0) for i, w in enumerate(WIDTHS) for j, nv in enumerate(VARIANTS) for k, P in enumerate(PERMS)]


@pytest.mark.parametrize("width,nv,n_perms,strict", CASES)
def test_counts_and_statistics(width, nv, n_perms, strict):
    c = _case(width, nv, n_perms, strict)
    e = _engine(c)
    counts, n_ge, bmax, pc = _run_dev(e, c)
    e.close()
    obs, perm = c["obs"], c["perm"]
    assert np.array_equal(counts, obs)
    # counts, bit-exact, under every relabelling; the unaffected side by difference from the observed row totals
    assert np.array_equal(pc[:, :, 0], perm[:, :, 0]) and np.array_equal(pc[:, :, 1], perm[:, :, 1])
    R1, R2 = obs[:, 0] + obs[:, 2], obs[:, 1] + obs[:, 3]
    assert np.array_equal(R1[:, None] - pc[:, :, 0], perm[:, :, 2]) and np.array_equal(R2[:, None] - pc[:, :, 1], perm[:, :, 3])
    assert np.array_equal(pc[:, 0, :], counts[:, :2])                   # row 0 is the observed labelling
    # statistics, exact
    exp_ge, exp_max, t_obs = _reference(width, nv, n_perms, strict)
    assert np.array_equal(n_ge, exp_ge)
    assert np.array_equal(bmax.view(np.uint64), exp_max.view(np.uint64))
    assert np.all(n_ge[np.isnan(t_obs)] == 0)
    if nv >= 3:
        assert np.isnan(t_obs[1]) and np.isnan(t_obs[2])
    # and against the oracle's own arithmetic
    chi_orc = orc.assoc_stats(orc.TASK_CHISQ, *[perm[:, :, k].reshape(-1) for k in range(4)])[1].reshape(nv, n_perms)
    assert_close(bmax, np.fmax.reduce(chi_orc, axis=0, initial=0.0), "batch_max")


MID = ((37, 45), 150, 33, False)


def _text(codes, is_x):
    a1, a2 = codes >> 4, codes & 15
    names = np.array([str(i) for i in range(15)] + ["."])
    cells = np.char.add(np.char.add(names[a1], "/"), names[a2])
    return "".join("%s\t%d\trs%d\tA\tC,G,T\t.\tPASS\t.\tGT\t%s\n" % ("X" if is_x[v] else "7", 100 + v, v, "\t".join(cells[v]))
                   for v in range(codes.shape[0])).encode()


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_host_and_text_entry_points():
    c = _case(*MID)
    exp_ge, exp_max, _ = _reference(*MID)
    e = _engine(c)
    res = e.assoc_perm(c["codes"], c["is_x"])
    assert np.array_equal(res["n_ge"], exp_ge) and np.array_equal(res["batch_max"].view(np.uint64), exp_max.view(np.uint64))
    _same(res, e.assoc(hpgv.TASK_CHISQ, c["codes"], c["is_x"]), ("A1", "A2", "U1", "U2", "odds", "chisq", "p"))
    text = _text(c["codes"], c["is_x"])
    rt = e.assoc_perm_text(text)
    assert rt["n_lines"] == c["nv"] and not rt["status"].any()
    assert np.array_equal(rt["n_ge"], exp_ge) and np.array_equal(rt["batch_max"].view(np.uint64), exp_max.view(np.uint64))
    _same(rt, e.assoc_text(hpgv.TASK_CHISQ, text), ("A1", "A2", "U1", "U2", "odds", "chisq", "p"))
    e.close()


def test_text_lines_that_are_no_records_take_no_part():
    c = _case(*MID)
    e = _engine(c)
    lines = _text(c["codes"], c["is_x"]).split(b"\n")[:-1]
    keep = np.ones(c["nv"], bool)
    keep[[0, 40, 149]] = False
    text = b"".join((l if keep[i] else b"7\t5\trs") + b"\n" for i, l in enumerate(lines))      # three lines cut short
    rt = e.assoc_perm_text(text)
    sub = dict(c, codes=c["codes"][keep], is_x=c["is_x"][keep])
    _, n_ge, bmax, _ = _run_dev(e, sub)
    e.close()
    assert rt["n_lines"] == c["nv"] and np.array_equal(rt["status"] != 0, ~keep)
    assert np.array_equal(rt["n_ge"][keep], n_ge) and not rt["n_ge"][~keep].any()
    assert np.array_equal(rt["batch_max"].view(np.uint64), bmax.view(np.uint64))


def test_splitting_the_variants_merges_by_maximum():
    c = _case(*MID)
    exp_ge, exp_max, _ = _reference(*MID)
    e = _engine(c)
    parts = [_run_dev(e, c, rows) for rows in (slice(0, 50), slice(50, 51), slice(51, 150))]
    empty = _run_dev(e, c, slice(0, 0))
    e.close()
    assert np.array_equal(np.concatenate([p[1] for p in parts]), exp_ge)
    assert np.array_equal(np.maximum.reduce([p[2] for p in parts]).view(np.uint64), exp_max.view(np.uint64))
    assert not empty[2].any()                            # no variants: the identity of the merge


def test_group_context():
    c = _case(*MID)
    exp_ge, exp_max, _ = _reference(*MID)
    g = _engine(c, [0, 0])
    for _ in range(2):                                   # dealt to one member, then the other
        res = g.assoc_perm(c["codes"], c["is_x"])
        assert np.array_equal(res["n_ge"], exp_ge) and np.array_equal(res["batch_max"].view(np.uint64), exp_max.view(np.uint64))
    rt = g.assoc_perm_text(_text(c["codes"], c["is_x"]))
    assert np.array_equal(rt["n_ge"], exp_ge) and np.array_equal(rt["batch_max"].view(np.uint64), exp_max.view(np.uint64))
    _, n_ge, bmax, _ = _run_dev(g.member(0), c)
    assert np.array_equal(n_ge, exp_ge) and np.array_equal(bmax.view(np.uint64), exp_max.view(np.uint64))
    g.close()


def test_label_state():
    c = _case(*MID)
    exp_ge, exp_max, _ = _reference(*MID)
    e = hpgv.Engine(0)
    e.set_cohort(c["cond"])
    d = e.alloc(4096)
    dev_call = lambda: e.L.hpgv_assoc_perm_dev(e.h, d, 0, None, d, d, d, None, None)
    assert dev_call() == hpgv.ERR_STATE
    with pytest.raises(hpgv.HpgvError, match="hpgv error %d" % hpgv.ERR_STATE):
        e.assoc_perm(c["codes"], c["is_x"])
    bad = c["labels"].copy()
    bad[3, np.flatnonzero(c["cond"] != 2)[5]] = 2
    lab = np.ascontiguousarray(bad)
    assert e.L.hpgv_set_perm_labels(e.h, C.c_void_p(lab.ctypes.data), len(lab)) == hpgv.ERR_INVALID
    assert dev_call() == hpgv.ERR_STATE
    bad[3] = c["labels"][3]
    bad[:, c["cond"] == 2] = 9                           # columns outside the cohort may hold anything
    e.set_perm_labels(bad)
    for _ in range(2):                                   # the labels survive consecutive calls
        res = e.assoc_perm(c["codes"], c["is_x"])
        assert np.array_equal(res["n_ge"], exp_ge) and np.array_equal(res["batch_max"].view(np.uint64), exp_max.view(np.uint64))
    e.set_perm_labels(None)                              # n_perms == 0 drops them
    assert dev_call() == hpgv.ERR_STATE
    e.set_perm_labels(c["labels"])
    assert dev_call() == hpgv.OK
    e.set_cohort(c["cond"])                              # so does a new cohort
    assert dev_call() == hpgv.ERR_STATE
    e.close()
