"""Family-flip permutation of the TDT (k_tdt_perm, csrc/hpgv_tdt_perm_kernels.h).  The reference is built here from the unchanged
oracle: orc.tdt_counts once per family with a one-family pedigree gives (t1_f, t2_f) of every variant, the flipped sums are
formed in numpy, orc.tdt_stats gives the chi-square.  Both sides divide the same two integers once in f64, so nothing has a
tolerance: perm_tu and n_ge equal, batch_max bit-identical, EMP1 / EMP2 equal to hpgv_perm_pvalues of the reference's inputs."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import assert_p_close, hpgv, random_codes
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

# (fast trios, slow families, variants, permutations).  Fast: none, under one 16-byte chunk, exactly one, past one 64-byte
# k-step (70 -> 5 chunks, 300 -> 19).  Slow: none, under one chunk, past one.  Variants: one, a ragged second workgroup, a
# ragged third.  Permutations: one, a ragged 16-column tile, a ragged second workgroup column.
CASES = [(0, 3, 65, 17), (5, 0, 1, 1), (16, 3, 65, 17), (70, 20, 130, 130), (300, 0, 65, 130), (300, 20, 130, 17)]
MID = (70, 20, 130, 130)


def _pedigree(rng, n_fast, n_slow, slow_children=None):
    """families in random order: n_fast with one child, n_slow with two or three (or slow_children each), three whose father is
    no VCF column and one without children (the plan skips those four); returns (n_samples, CSR arrays of hpgv_set_families)"""
    kinds = [1] * n_fast + [slow_children or int(rng.integers(2, 4)) for _ in range(n_slow)] + [-1, -1, -2, 0]
    kinds = [kinds[i] for i in rng.permutation(len(kinds))]
    n_samples = sum(2 + max(abs(k), 1) for k in kinds) + 7
    cols = [int(c) for c in rng.permutation(n_samples)]
    fcol, mcol, coff, ccol, csex = [], [], [0], [], []
    for k in kinds:
        f, m = cols.pop(), cols.pop()
        fcol.append(-1 if k < 0 else f)
        mcol.append(m)
        for _ in range(abs(k)):
            ccol.append(cols.pop())
            csex.append(int(rng.integers(0, 2)))
        coff.append(len(ccol))
    return n_samples, (np.array(fcol, np.int32), np.array(mcol, np.int32), np.array(coff, np.int32), np.array(ccol, np.int32),
                       np.array(csex, np.uint8))


def _family_counts(codes, fam, is_x):
    """(t1_f, t2_f) of every variant and family, [nv, n_families] each: the oracle on one-family pedigrees"""
    fcol, mcol, coff, ccol, csex = fam
    nv, nf = codes.shape[0], len(fcol)
    t1, t2 = np.zeros((nv, nf), np.int64), np.zeros((nv, nf), np.int64)
    for f in range(nf):
        a, b = coff[f], coff[f + 1]
        t1[:, f], t2[:, f] = orc.tdt_counts(codes, fcol[f:f + 1], mcol[f:f + 1], [0, b - a], ccol[a:b], csex[a:b], chrom_is_x=is_x)
    return t1, t2


def _chisq(t1, t2):
    return orc.tdt_stats(np.asarray(t1).reshape(-1), np.asarray(t2).reshape(-1))[1].reshape(np.shape(t1))


@functools.lru_cache(maxsize=None)
def _case(n_fast, n_slow, nv, n_perms, special=(), no_part=()):
    """special: further special flip rows, (row, kind) with kind "none" or "all", set after the fixed ones; no_part: further
    variants with every parent homozygous"""
    rng = np.random.default_rng(100000 * n_fast + 1000 * n_slow + 10 * nv + n_perms)
    ns, fam = _pedigree(rng, n_fast, n_slow)
    nf = len(fam[0])
    # half the rows from every genotype string the rules know (Mendel errors, missing and multi-allelic calls), half a realistic
    # mix with many counted trios
    codes = random_codes(rng, nv, ns, quirks=True)
    codes[nv // 2:] = random_codes(rng, nv - nv // 2, ns, quirks=False)
    is_x = (rng.random(nv) < 0.35).astype(np.uint8)
    if nv >= 3:
        codes[1] = 0x00                                  # every parent homozygous: t1 + t2 == 0
        is_x[0], is_x[nv - 1] = 0, 1
    for v in no_part:
        codes[v] = 0x00
    flips = (rng.random((n_perms, nf)) < rng.uniform(0.2, 0.8, size=(n_perms, 1))).astype(np.uint8)
    flips[0] = 0                                         # the observed transmission
    if n_perms >= 17:
        flips[n_perms - 1] = 1                           # every family flipped
    for row, kind in special:
        flips[row] = {"none": 0, "all": 1}[kind]
    return _finish(ns, fam, codes, is_x, flips, n_fast, n_slow)


def _finish(ns, fam, codes, is_x, flips, n_fast, n_slow):
    """the case of a pedigree, a code matrix and flip rows: the reference's tallies, permuted tallies, n_ge and batch_max"""
    nf, (nv, n_perms) = len(fam[0]), (codes.shape[0], flips.shape[0])
    t1f, t2f = _family_counts(codes, fam, is_x)
    F = flips.astype(np.int64).T                         # [nf, P]
    t1p, t2p = t1f @ (1 - F) + t2f @ F, t2f @ (1 - F) + t1f @ F
    obs = orc.tdt_counts(codes, *fam, chrom_is_x=is_x)
    assert np.array_equal(t1f.sum(axis=1), obs[0]) and np.array_equal(t2f.sum(axis=1), obs[1])      # the families add up
    chi_obs, chi = _chisq(*obs), _chisq(t1p, t2p)
    part = (obs[0] + obs[1]) > 0                         # the variants that take part
    n_ge = np.where(part, (chi >= chi_obs[:, None]).sum(axis=1), 0).astype(np.int32)
    bmax = np.max(np.where(part[:, None], chi, 0.0), axis=0, initial=0.0)
    c = dict(ns=ns, fam=fam, nf=nf, codes=codes, is_x=is_x, flips=flips, t1=obs[0], t2=obs[1], chi_obs=chi_obs, part=part,
             perm_tu=np.stack([t1p, t2p], axis=2).astype(np.int32), n_ge=n_ge, bmax=bmax, nv=nv, n_perms=n_perms,
             n_fast=n_fast, n_slow=n_slow, d_f=t1f - t2f)
    for a in (codes, is_x, flips, c["perm_tu"], n_ge, bmax):
        a.setflags(write=False)
    return c


def _engine(c, device=0):
    e = hpgv.Engine(device)
    assert e.set_families(c["ns"], *c["fam"])[:2] == (c["n_fast"], c["n_slow"])
    e.set_tdt_flips(c["flips"])
    return e


def _run_dev(e, c, rows=slice(None)):
    """layout, scan and the permutation kernels on device buffers: (tu, n_ge, batch_max, perm_tu)"""
    codes, is_x = np.ascontiguousarray(c["codes"][rows]), np.ascontiguousarray(c["is_x"][rows])
    nv, P, ns = len(codes), c["n_perms"], c["ns"]
    pitch = e.tdt_layout()[2]
    bufs = [e.alloc(max(n, 16)) for n in (nv * ns, nv * pitch, nv * 8, nv * 4, P * 8, nv * P * 8, nv)]
    d_raw, d_lay, d_tu, d_nge, d_bmax, d_pt, d_x = bufs
    e.h2d(d_bmax, np.full(P, 7.0))                       # overwritten, not merged into
    if nv:
        e.h2d(d_raw, codes)
        e.h2d(d_x, is_x)
        e.h2d(d_nge, np.full(nv, 9, np.int32))
        e.layout(hpgv.LAYOUT_TDT, d_raw, ns, nv, d_lay)
        e.tdt_scan(d_lay, nv, d_tu, d_x)
    e.tdt_perm_dev(d_lay, nv, d_tu, d_nge, d_bmax, d_pt, d_x)
    e.sync()
    get = lambda d, shape, dtype: e.d2h(d, shape, dtype) if nv else np.zeros(shape, dtype)
    out = (get(d_tu, (nv, 2), np.int32), get(d_nge, (nv,), np.int32), e.d2h(d_bmax, (P,), np.float64), get(d_pt, (nv, P, 2), np.int32))
    for b in bufs:
        e.free(b)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check(res, c, what):
    assert np.array_equal(res["n_ge"], c["n_ge"]), what
    assert np.array_equal(_bits(res["batch_max"]), _bits(c["bmax"])), what


@pytest.mark.parametrize("n_fast,n_slow,nv,n_perms", CASES)
def test_counts_and_statistics(n_fast, n_slow, nv, n_perms):
    c = _case(n_fast, n_slow, nv, n_perms)
    e = _engine(c)
    tu, n_ge, bmax, pt = _run_dev(e, c)
    e.close()
    assert np.array_equal(tu[:, 0], c["t1"]) and np.array_equal(tu[:, 1], c["t2"])
    assert np.array_equal(pt, c["perm_tu"])
    assert np.array_equal(n_ge, c["n_ge"])
    assert np.array_equal(_bits(bmax), _bits(c["bmax"]))
    # the all-zero flip row is the observed transmission: it reaches the observed statistic wherever there is one
    assert np.array_equal(pt[:, 0, :], tu)
    assert np.all(n_ge[c["part"]] >= 1) and not n_ge[~c["part"]].any()
    if n_perms >= 17:                                    # every family flipped: the two counts change places
        assert np.array_equal(pt[:, n_perms - 1, :], tu[:, ::-1])
    if nv >= 3:
        assert not c["part"][1] and c["part"].sum() > nv // 4
    # the p-values of the engine's outputs are those of the reference's inputs
    t_eng = np.where(c["part"], _chisq(tu[:, 0], tu[:, 1]), np.nan)
    t_ref = np.where(c["part"], c["chi_obs"], np.nan)
    got, exp = hpgv.perm_pvalues(t_eng, n_ge, bmax), hpgv.perm_pvalues(t_ref, c["n_ge"], c["bmax"])
    assert np.array_equal(got[0], exp[0], equal_nan=True) and np.array_equal(got[1], exp[1], equal_nan=True)
    assert np.isnan(exp[0][~c["part"]]).all()


def test_tdt_outputs_stay_those_of_the_oracle():
    """hpgv_tdt on the same inputs, through the one-pass kernel and through the kernel chain: tallies, odds and chi-square are the
    oracle's bit for bit (tdt_chisq_value is k_tdt_stats' arithmetic moved, not changed).  The p-value is chisq_p_value of that
    chi-square, a function this file's subject does not touch: the engine's erfc and the oracle's differ in the last digits
    (7e-15 relative on this case, before the move as after), so p is held to the suite's p-value bounds"""
    c = _case(*MID)
    odds, chisq, p = orc.tdt_stats(c["t1"], c["t2"])
    for fused in (1, 0):
        e = _engine(c)
        e.set_option("batch_fused", fused)
        for res in (e.tdt(c["codes"], c["is_x"]), e.tdt_perm(c["codes"], c["is_x"])):
            assert np.array_equal(res["t1"], c["t1"]) and np.array_equal(res["t2"], c["t2"])
            assert np.array_equal(_bits(res["chisq"]), _bits(chisq)), fused
            assert np.array_equal(_bits(res["odds"]), _bits(odds)), fused
            assert_p_close(res["p"], p, "tdt p")
        e.close()


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
    e = _engine(c)
    res = e.tdt_perm(c["codes"], c["is_x"])
    _check(res, c, "host")
    _same(res, e.tdt(c["codes"], c["is_x"]), ("t1", "t2", "odds", "chisq", "p"))
    text = _text(c["codes"], c["is_x"])
    rt = e.tdt_perm_text(text)
    assert rt["n_lines"] == c["nv"] and not rt["status"].any()
    _check(rt, c, "text")
    _same(rt, e.tdt_text(text), ("t1", "t2", "odds", "chisq", "p"))
    e.close()


def test_text_lines_that_are_no_records_take_no_part():
    c = _case(*MID)
    e = _engine(c)
    lines = _text(c["codes"], c["is_x"]).split(b"\n")[:-1]
    keep = np.ones(c["nv"], bool)
    keep[[0, 40, int(np.argmax(c["chi_obs"])), c["nv"] - 1]] = False
    text = b"".join((l if keep[i] else b"7\t5\trs") + b"\n" for i, l in enumerate(lines))      # four lines cut short
    rt = e.tdt_perm_text(text)
    sub = dict(c, codes=c["codes"][keep], is_x=c["is_x"][keep])
    _, n_ge, bmax, _ = _run_dev(e, sub)
    e.close()
    assert rt["n_lines"] == c["nv"] and np.array_equal(rt["status"] != 0, ~keep)
    assert np.array_equal(rt["n_ge"][keep], n_ge) and not rt["n_ge"][~keep].any()
    assert np.array_equal(rt["n_ge"][keep], c["n_ge"][keep])
    assert np.array_equal(_bits(rt["batch_max"]), _bits(bmax))


def test_splitting_the_variants_merges_by_maximum():
    c = _case(*MID)
    e = _engine(c)
    parts = [_run_dev(e, c, rows) for rows in (slice(0, 50), slice(50, 51), slice(51, 130))]
    empty = _run_dev(e, c, slice(0, 0))
    e.close()
    assert np.array_equal(np.concatenate([p[1] for p in parts]), c["n_ge"])
    assert np.array_equal(_bits(np.maximum.reduce([p[2] for p in parts])), _bits(c["bmax"]))
    assert not empty[2].any()                            # no variants: the identity of the merge


def test_group_context():
    c = _case(*MID)
    g = _engine(c, [0, 0])
    for _ in range(2):                                   # dealt to one member, then the other
        _check(g.tdt_perm(c["codes"], c["is_x"]), c, "group host")
    _check(g.tdt_perm_text(_text(c["codes"], c["is_x"])), c, "group text")
    _, n_ge, bmax, _ = _run_dev(g.member(0), c)
    _check(dict(n_ge=n_ge, batch_max=bmax), c, "group member")
    g.close()


def test_flip_state():
    c = _case(*MID)
    e = hpgv.Engine(0)
    d = e.alloc(4096)
    flips = np.ascontiguousarray(c["flips"])
    set_raw = lambda a: e.L.hpgv_set_tdt_flips(e.h, C.c_void_p(a.ctypes.data), len(a))
    assert set_raw(flips) == hpgv.ERR_STATE             # flips before families
    e.set_families(c["ns"], *c["fam"])
    dev_call = lambda: e.L.hpgv_tdt_perm_dev(e.h, d, 0, None, d, d, d, None, None)
    assert dev_call() == hpgv.ERR_STATE
    with pytest.raises(hpgv.HpgvError, match="hpgv error %d" % hpgv.ERR_STATE):
        e.tdt_perm(c["codes"], c["is_x"])
    counted = np.flatnonzero((c["fam"][0] >= 0) & (np.diff(c["fam"][2]) > 0))
    skipped = np.setdiff1d(np.arange(c["nf"]), counted)
    bad = c["flips"].copy()
    bad[3, counted[5]] = 2
    assert set_raw(bad) == hpgv.ERR_INVALID
    assert dev_call() == hpgv.ERR_STATE
    bad[3] = c["flips"][3]
    bad[:, skipped] = 9                                  # families the plan skips may hold anything
    e.set_tdt_flips(bad)
    for _ in range(2):                                   # the flips survive consecutive calls
        _check(e.tdt_perm(c["codes"], c["is_x"]), c, "state")
    e.set_tdt_flips(None)                                # n_perms == 0 drops them
    assert dev_call() == hpgv.ERR_STATE
    e.set_tdt_flips(c["flips"])
    assert dev_call() == hpgv.OK
    e.set_families(c["ns"], *c["fam"])                   # so do new families
    assert dev_call() == hpgv.ERR_STATE
    # a family of 64 counted children: |d_f| up to 128 does not fit the i8 operand
    e.set_families(70, [0, 2], [1, 3], [0, 64, 65], list(range(4, 69)), [0] * 65)
    one = np.zeros((1, 2), np.uint8)
    assert set_raw(one) == hpgv.ERR_UNSUPPORTED
    e.set_families(70, [0, 2], [1, 3], [0, 63, 64], list(range(4, 68)), [0] * 64)      # 63 fit
    assert set_raw(one) == hpgv.OK
    e.free(d)
    e.close()
