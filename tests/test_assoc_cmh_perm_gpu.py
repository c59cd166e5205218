"""Permutation within strata on the device (k_assoc_cmh_perm, csrc/hpgv_assoc_cmh_perm_kernels.h): T_p of every (variant,
permutation) bit for bit hpgv_cmh_fit's chisq of the golden's permuted tables and within TOL of the exact rationals, NaN where the
definition says, n_ge and batch_max exactly what those T_p imply, pieces and repeats byte for byte, the batch and text entry points,
the state rules.

The cohort is 150 cohort columns + 7 HPGV_COND_OTHER columns (three k-steps, the last partial).  Strata: K = 1; K = 3 interleaved
with four cohort columns in none; K = 5 in blocks (step lists that skip k-steps); K = 70 (2K passes one image tile) -- all but K = 1,
which has only its one stratum, with a single-sample stratum and an all-affected one.  With 10 % missing calls and with none (every
within-strata row then takes the kernel's shortcut).  Rows: all missing, monomorphic, chr X.  The rationals are evaluated on a fixed
sample of the pairs of each case and on every pair hpgv_cmh_fit calls NaN; hpgv_cmh_fit itself is compared on every pair."""
import numpy as np
import pytest

import cmh_golden as cg
import cmh_perm_golden as pg
from helpers import assert_close, hpgv

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (64, 128), (65, 129), (130, 300), (1, 300), (130, 1)]      # (variants, permutations): tiles of 64 x passes of 64
CASES = [(kind, missing, nv, P) for kind in pg.STRATA for missing in (0.1, 0.0) for nv, P in SHAPES]
MID = ("five_blocks", 0.1)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("kind,missing,nv,P", CASES)
def test_every_permuted_statistic_and_what_follows_from_it(kind, missing, nv, P):
    c = pg.base(kind, missing)
    e = pg.engine(c, P)
    out, n_ge, bmax, t = pg.run_dev(e, c, nv, P)
    e.close()
    want = c["t_perm"][:nv, :P]
    assert _same_bits(out["chisq"], c["t_obs"][:nv])                                      # T_obs is the record's chisq
    assert _same_bits(t, want)                                                            # NaN exactly where the definition says
    assert not np.isinf(t).any()
    if nv >= 3:
        assert np.isnan(t[1]).all() and np.isnan(t[2]).all()                              # all missing; monomorphic
    assert _same_bits(t[:, 0], out["chisq"])                                              # label row 0 is the observed labelling
    # the rationals: a fixed sample of the pairs
    rng = np.random.default_rng(nv * 1000 + P)
    pairs = {(int(v), int(p)) for v, p in zip(rng.integers(0, nv, 60), rng.integers(0, P, 60))} | {(0, 0), (nv - 1, P - 1), (min(1, nv - 1), P - 1)}
    for v, p in sorted(pairs):
        assert_close(t[v, p], pg.rational_chisq(c["perm_tables"][v, p]), "T_p(%d, %d)" % (v, p))
    exp_ge, exp_max = pg.expected(c, nv, P)
    assert np.array_equal(n_ge, exp_ge)
    assert np.array_equal(_bytes(bmax), _bytes(exp_max))
    if nv >= 64 and P >= 128:
        assert n_ge.max() > 1 and (bmax > 0).all() and 0 < (n_ge == 0).sum()


def _same_bits(a, b):
    """NaN in the same places, every other value bit for bit"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


@pytest.mark.parametrize("kind", pg.STRATA)
def test_pieces_an_empty_call_and_two_runs_give_the_same_bytes(kind):
    c = pg.base(kind, 0.1)
    nv, P = 130, 129
    e = pg.engine(c, P)
    whole = pg.run_dev(e, c, nv, P)
    again = pg.run_dev(e, c, nv, P, want_chisq=False)
    parts = [pg.run_dev(e, c, nv, P, rows) for rows in (slice(0, 65), slice(65, 66), slice(66, 130))]
    empty = pg.run_dev(e, c, nv, P, slice(0, 0))
    e.close()
    assert np.array_equal(again[1], whole[1]) and np.array_equal(_bytes(again[2]), _bytes(whole[2]))
    assert np.array_equal(np.concatenate([q[1] for q in parts]), whole[1])
    assert np.array_equal(_bytes(np.concatenate([q[3] for q in parts])), _bytes(whole[3]))
    assert np.array_equal(_bytes(np.maximum.reduce([q[2] for q in parts])), _bytes(whole[2]))      # batch_max merges by maximum
    for q, rows in zip(parts, (slice(0, 65), slice(65, 66), slice(66, 130))):
        assert np.array_equal(_bytes(q[2]), _bytes(pg.expected(c, nv, P, rows)[1]))
    assert len(empty[1]) == 0 and not empty[2].any()                                               # no variants: batch_max 0.0


def test_batch_and_text_calls_equal_the_device_call():
    c = pg.base(*MID)
    nv, P = 17, 70
    e = pg.engine(c, P)
    dev_out, dev_ge, dev_max, _ = pg.run_dev(e, c, nv, P, want_chisq=False)
    codes, is_x = c["codes"][:nv], c["is_x"][:nv]
    plain = e.assoc_cmh(codes, is_x)
    res = e.assoc_cmh_perm(codes, is_x)
    assert np.array_equal(_bytes(res["out"]), _bytes(plain)) and np.array_equal(_bytes(plain), _bytes(dev_out))
    assert np.array_equal(res["n_ge"], dev_ge) and np.array_equal(_bytes(res["batch_max"]), _bytes(dev_max))
    none = e.assoc_cmh_perm(codes[:0], is_x[:0])
    assert len(none["out"]) == 0 and none["batch_max"].shape == (P,) and not none["batch_max"].any()
    # the text: rows on chromosome 7 and on X as the tokenizer flags them, a header line and a damaged line among them
    lines = [cg.text_of(codes[v:v + 1], "X" if is_x[v] else "7").replace(b"\t100\t", b"\t%d\t" % (100 + v)) for v in range(nv)]
    text = b"".join(lines[:5]) + b"##a header line\n" + b"".join(lines[5:11]) + b"7\t55\n" + b"".join(lines[11:])
    HEADER, DAMAGED = 5, 12
    mark = np.zeros(nv + 3, hpgv.CMH_RESULT)
    mark["chisq"], mark["n_strata_bd"] = -7.0, -7
    txt = e.assoc_cmh_perm_text(text, out=mark.copy())
    ref = e.assoc_cmh_text(text)
    e.close()
    assert txt["n_lines"] == nv + 2
    rec = np.ones(nv + 2, bool)
    rec[[HEADER, DAMAGED]] = False
    assert (txt["status"][~rec] & 0xFF).all() and not (txt["status"][rec] & 0xFF).any()
    assert np.array_equal(_bytes(txt["out"][rec]), _bytes(dev_out)) and np.array_equal(_bytes(txt["out"][rec]), _bytes(ref["out"][rec]))
    assert np.array_equal(_bytes(txt["out"][~rec]), _bytes(mark[:nv + 2][~rec]))                   # skipped: the record untouched,
    assert np.array_equal(txt["n_ge"][rec], dev_ge) and not txt["n_ge"][~rec].any()                # n_ge 0,
    assert np.array_equal(_bytes(txt["batch_max"]), _bytes(dev_max))                               # and no part in the maxima


def test_a_text_of_skipped_lines_only_gives_zero_maxima():
    c = pg.base(*MID)
    e = pg.engine(c, 5)
    txt = e.assoc_cmh_perm_text(b"##only a header\n7\t55\n")
    e.close()
    assert txt["n_lines"] == 2 and not txt["n_ge"].any() and txt["batch_max"].shape == (5,) and not txt["batch_max"].any()


def test_state_rules():
    c = pg.base(*MID)
    e = hpgv.Engine(0)
    d = e.alloc(4096)
    dev_call = lambda: e.L.hpgv_assoc_cmh_perm_dev(e.h, d, 0, None, d, d, d, None, None)
    e.set_cohort(c["cond"])
    assert dev_call() == hpgv.ERR_STATE                              # neither
    e.set_strata(c["stratum"], c["K"])
    assert dev_call() == hpgv.ERR_STATE                              # no labels
    with pytest.raises(hpgv.HpgvError, match="hpgv error %d" % hpgv.ERR_STATE):
        e.assoc_cmh_perm(c["codes"][:3])
    with pytest.raises(hpgv.HpgvError, match="hpgv error %d" % hpgv.ERR_STATE):
        e.assoc_cmh_perm_text(cg.text_of(c["codes"][:3]))
    e.set_perm_labels(c["labels"][:9])
    assert dev_call() == hpgv.OK
    e.set_strata(None)
    assert dev_call() == hpgv.ERR_STATE                              # no strata
    with pytest.raises(hpgv.HpgvError, match="hpgv error %d" % hpgv.ERR_STATE):
        e.assoc_cmh_perm(c["codes"][:3])
    e.set_strata(c["stratum"], c["K"])
    assert dev_call() == hpgv.OK
    assert e.L.hpgv_assoc_cmh_perm_dev(e.h, d, -1, None, d, d, d, None, None) == hpgv.ERR_INVALID
    assert e.L.hpgv_assoc_cmh_perm_dev(e.h, d, 1, None, None, d, d, None, None) == hpgv.ERR_INVALID
    assert e.L.hpgv_assoc_cmh_perm_dev(e.h, d, 1, None, d, d, None, None, None) == hpgv.ERR_INVALID
    off = lambda n: type(d)(d.value + n)
    assert e.L.hpgv_assoc_cmh_perm_dev(e.h, off(8), 1, None, d, d, d, None, None) == hpgv.ERR_INVALID      # d_gt not 16-byte aligned
    assert e.L.hpgv_assoc_cmh_perm_dev(e.h, d, 1, None, d, d, off(4), None, None) == hpgv.ERR_INVALID      # d_batch_max not 8-byte aligned
    e.set_cohort(c["cond"])                                          # a new cohort drops both
    assert dev_call() == hpgv.ERR_STATE
    e.close()


def test_a_group_context_deals_the_call():
    c = pg.base(*MID)
    nv, P = 17, 70
    e = pg.engine(c, P)
    want = e.assoc_cmh_perm(c["codes"][:nv], c["is_x"][:nv])
    e.close()
    g = pg.engine(c, P, device=[0, 0])
    for _ in range(3):                                               # both members take a call
        got = g.assoc_cmh_perm(c["codes"][:nv], c["is_x"][:nv])
        assert all(np.array_equal(_bytes(got[k]), _bytes(want[k])) for k in ("out", "n_ge", "batch_max"))
    g.close()
