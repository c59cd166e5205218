"""Stratified association on the device (k_assoc_cmh_tables<1, 2, 4, 8> and k_assoc_cmh_stats, csrc/hpgv_assoc_cmh_kernels.h): the
per-stratum allele tables off the matrix cores exact against numpy's plane products, the records within TOL of cmh_golden's
oracles, the identities of include/hpgv.h "stratified association", pieces and repeats bit for bit, the strata state, the label
state beside it, and the batch and text entry points."""
import numpy as np
import pytest

import cmh_golden as cg
from helpers import TOL, assert_close, assert_p_close, close, hpgv

pytestmark = pytest.mark.gpu

WIDTHS = [(2, 3), (37, 45), (64, 64), (301, 412)]      # (affected, unaffected): 5 columns; two ragged k-steps; whole chunks; 12 k-steps, the last ragged
VARIANTS = [1, 17, 150]                                 # one row; a ragged 16-row tile; three workgroups, the last ragged
STRATA = [1, 2, 9, 20, 40, 70]                          # NT = 1 (a ragged tile), 1, 2 (ragged), 4 (ragged), 8 (ragged), 8 in two passes with a ragged last one
CASES = [(w, nv, K) for i, w in enumerate(WIDTHS) for j, nv in enumerate(VARIANTS) for k, K in enumerate(STRATA) if (i + j + k) % 2 == 0]


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _check_records(got, ref, what=""):
    assert np.array_equal(got["n_strata_cmh"], ref["n_strata_cmh"]) and np.array_equal(got["n_strata_bd"], ref["n_strata_bd"]), what
    for k in cg.FIELDS:
        (assert_p_close if k in ("p", "p_bd") else assert_close)(got[k], ref[k], "%s %s" % (what, k))
        assert not np.isinf(got[k]).any(), (what, k)


@pytest.mark.parametrize("width,nv,K", CASES)
def test_tables_and_records(width, nv, K):
    c = cg.case(width, nv, K, quirks=(nv + K) % 4 != 1)
    e = cg.engine(c)
    out, tab = cg.run_dev(e, c)
    out2, _ = cg.run_dev(e, c, own_tables=False)                     # the tables in the context's scratch
    e.close()
    assert np.array_equal(tab, c["tables"])
    _check_records(out, c["ref"])
    assert np.array_equal(_bytes(out), _bytes(out2))
    if nv >= 3:
        assert np.isnan(out["chisq"][1]) and np.isnan(out["chisq"][2]) and out["n_strata_cmh"][1] == 0      # all missing; monomorphic
    # relabelling the strata by a permutation: the tables move with it, the records stay within TOL
    perm = np.random.default_rng(K).permutation(K)
    e = hpgv.Engine(0)
    e.set_cohort(c["cond"])
    e.set_strata(np.where(c["stratum"] >= 0, perm[np.clip(c["stratum"], 0, K - 1)], -1).astype(np.int32), K)
    out3, tab3 = cg.run_dev(e, c)
    e.close()
    assert np.array_equal(tab3[:, perm], c["tables"])
    _check_records(out3, c["ref"], "relabelled")


MID = ((37, 45), 150, 9)


def test_pieces_an_empty_call_and_two_runs_give_the_same_bytes():
    c = cg.case(*MID)
    e = cg.engine(c)
    whole, tab = cg.run_dev(e, c)
    again, tab_again = cg.run_dev(e, c)
    parts = [cg.run_dev(e, c, rows) for rows in (slice(0, 50), slice(50, 51), slice(51, 150))]
    empty, empty_tab = cg.run_dev(e, c, slice(0, 0))
    e.close()
    assert np.array_equal(_bytes(whole), _bytes(again)) and np.array_equal(tab, tab_again)
    assert np.array_equal(_bytes(np.concatenate([p[0] for p in parts])), _bytes(whole))
    assert np.array_equal(np.concatenate([p[1] for p in parts]), tab)
    assert len(empty) == 0 and len(empty_tab) == 0


@pytest.mark.parametrize("width,nv", [((37, 45), 150), ((301, 412), 17)])
def test_one_stratum_is_the_allelic_test(width, nv):
    """K = 1 with the whole cohort in it: CHISQ_CMH = (n - 1) / n x hpgv_assoc's chi-square, OR_MH its odds ratio (which is 0, not
    NaN, where a d = 0 < b c: there sum R == 0 makes OR_MH NaN by the definition)"""
    c = cg.case(width, nv, 1, everyone=True)
    e = cg.engine(c)
    out, tab = e.assoc_cmh(c["codes"], c["is_x"], tables=True)
    ref = e.assoc(hpgv.TASK_CHISQ, c["codes"], c["is_x"])
    e.close()
    counts = np.stack([ref[k] for k in ("A1", "A2", "U1", "U2")], axis=1)
    assert np.array_equal(tab[:, 0, :], counts)
    n = counts.sum(axis=1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert_close(out["chisq"], (n - 1) / n * ref["chisq"], "chisq")
    has_r = (counts[:, 0].astype(np.int64) * counts[:, 3]) > 0
    assert has_r.sum() >= nv // 2
    assert_close(out["or_mh"][has_r], ref["odds"][has_r], "or_mh")
    assert np.isnan(out["or_mh"][~has_r]).all()
    assert np.isnan(out["chisq_bd"]).all() and (out["n_strata_bd"] <= 1).all()


@pytest.mark.parametrize("K", [2, 9, 70])
def test_the_strata_sum_to_the_scan(K):
    """every cohort sample in a stratum: sum_k tables[v, k] is hpgv_assoc_scan_dev's count, exactly"""
    c = cg.case((37, 45), 150, K, everyone=True)
    e = cg.engine(c)
    _, tab = cg.run_dev(e, c)
    nv, ns, pitch = c["nv"], c["ns"], e.assoc_layout()[2]
    d_raw, d_lay, d_x, d_c = e.alloc(nv * ns), e.alloc(nv * pitch), e.alloc(nv), e.alloc(nv * 16)
    e.h2d(d_raw, c["codes"])
    e.h2d(d_x, c["is_x"])
    e.layout(hpgv.LAYOUT_ASSOC, d_raw, ns, nv, d_lay)
    e.assoc_scan(d_lay, nv, d_c, d_x)
    e.sync()
    counts = e.d2h(d_c, (nv, 4), np.int32)
    e.close()
    assert np.array_equal(tab.sum(axis=1), counts)


@pytest.mark.parametrize("K", [2, 9, 70])
def test_a_common_odds_ratio_through_the_device(K):
    """genotype rows built from tables with a d = 2 b c in every stratum: OR_MH == 2, CHISQ_BD within TOL of 0, df = K - 1"""
    rng = np.random.default_rng(600 + K)
    nv = 5
    tabs = 2 * np.stack([cg.common_or_tables(rng, K) for _ in range(nv)])             # [nv, K, 4]: every cell even, a d = 2 b c still
    per = (tabs[:, :, 0::2] + tabs[:, :, 1::2]).max(axis=0) // 2                      # [K, class]: samples that carry the most alleles of any row
    cond = np.concatenate([np.full(per[k, g], 1 - g, np.uint8) for k in range(K) for g in range(2)])
    stratum = np.concatenate([np.full(per[k, g], k, np.int32) for k in range(K) for g in range(2)])
    codes = np.full((nv, len(cond)), 0xFF, np.uint8)                                  # hom-ref and hom-alt samples, the rest missing
    for v in range(nv):
        pos = 0
        for k in range(K):
            for g in range(2):
                cells = [0x00] * (int(tabs[v, k, 2 * g]) // 2) + [0x11] * (int(tabs[v, k, 2 * g + 1]) // 2)
                codes[v, pos:pos + len(cells)] = cells
                pos += per[k, g]
    order = rng.permutation(len(cond))                                                # the classes and strata interleaved
    cond, stratum, codes = cond[order], stratum[order], np.ascontiguousarray(codes[:, order])
    assert np.array_equal(cg.tables(codes, cond, stratum, K), tabs)
    e = hpgv.Engine(0)
    e.set_cohort(cond)
    e.set_strata(stratum, K)
    out, tab = e.assoc_cmh(codes, tables=True)
    e.close()
    assert np.array_equal(tab, tabs)
    assert (out["or_mh"] == 2.0).all()
    assert (np.abs(out["chisq_bd"]) <= TOL).all() and (out["n_strata_bd"] == K).all() and (out["n_strata_cmh"] == K).all()
    assert close(out["p_bd"], np.ones(nv))


def test_strata_state():
    c = cg.case(*MID)
    e = hpgv.Engine(0)
    d = e.alloc(4096)
    dev_call = lambda: e.L.hpgv_assoc_cmh_dev(e.h, d, 0, None, d, None, None)
    assert e.L.hpgv_set_strata(e.h, hpgv._ptr(c["stratum"]), c["ns"], c["K"]) == hpgv.ERR_STATE      # no cohort
    e.set_cohort(c["cond"])
    assert dev_call() == hpgv.ERR_STATE                              # no strata
    with pytest.raises(hpgv.HpgvError, match="hpgv error %d" % hpgv.ERR_STATE):
        e.assoc_cmh(c["codes"])
    with pytest.raises(hpgv.HpgvError, match="hpgv error %d" % hpgv.ERR_STATE):
        e.assoc_cmh_text(cg.text_of(c["codes"][:3]))
    e.set_strata(c["stratum"], c["K"])
    assert dev_call() == hpgv.OK
    e.set_strata(None)                                               # n_strata == 0 drops them
    assert dev_call() == hpgv.ERR_STATE
    e.set_strata(c["stratum"], c["K"])
    e.set_cohort(c["cond"])                                          # so does a new cohort
    assert dev_call() == hpgv.ERR_STATE
    cohort = np.flatnonzero(c["cond"] != 2)
    bad = c["stratum"].copy()
    bad[cohort[3]] = c["K"]                                          # a value >= n_strata in a cohort column
    assert e.L.hpgv_set_strata(e.h, hpgv._ptr(bad), c["ns"], c["K"]) == hpgv.ERR_INVALID
    assert e.L.hpgv_set_strata(e.h, hpgv._ptr(c["stratum"]), c["ns"] - 1, c["K"]) == hpgv.ERR_INVALID
    assert e.L.hpgv_set_strata(e.h, None, c["ns"], c["K"]) == hpgv.ERR_INVALID
    assert e.L.hpgv_set_strata(e.h, hpgv._ptr(c["stratum"]), c["ns"], -1) == hpgv.ERR_INVALID
    assert e.L.hpgv_set_strata(e.h, hpgv._ptr(c["stratum"]), c["ns"], hpgv.CMH_MAX_STRATA + 1) == hpgv.ERR_UNSUPPORTED
    assert dev_call() == hpgv.ERR_STATE                              # a refused call installs nothing
    e.set_strata(c["stratum"], hpgv.CMH_MAX_STRATA)                  # the limit itself: sixteen passes
    out, tab = e.assoc_cmh(c["codes"][:20], c["is_x"][:20], tables=True)
    assert np.array_equal(tab[:, :c["K"]], c["tables"][:20]) and not tab[:, c["K"]:].any()
    assert np.array_equal(out["n_strata_cmh"], c["ref"]["n_strata_cmh"][:20])
    e.close()


def test_the_permutation_labels_are_untouched():
    """hpgv_set_perm_labels, then hpgv_assoc_perm_dev before and after a CMH call: identical n_ge and batch_max"""
    c = cg.case(*MID)
    rng = np.random.default_rng(12)
    labels = (rng.random((33, c["ns"])) < 0.5).astype(np.uint8)
    e = hpgv.Engine(0)
    e.set_cohort(c["cond"])
    e.set_perm_labels(labels)
    e.set_strata(c["stratum"], c["K"])
    nv, ns, P, pitch = c["nv"], c["ns"], len(labels), e.assoc_layout()[2]
    d_raw, d_lay, d_x, d_c, d_nge, d_bmax = (e.alloc(n) for n in (nv * ns, nv * pitch, nv, nv * 16, nv * 4, P * 8))
    e.h2d(d_raw, c["codes"])
    e.h2d(d_x, c["is_x"])
    e.layout(hpgv.LAYOUT_ASSOC, d_raw, ns, nv, d_lay)
    e.assoc_scan(d_lay, nv, d_c, d_x)

    def perm():
        e.assoc_perm_dev(d_lay, nv, d_c, d_nge, d_bmax, None, d_x)
        e.sync()
        return e.d2h(d_nge, (nv,), np.int32), e.d2h(d_bmax, (P,), np.float64)

    before = perm()
    out, tab = cg.run_dev(e, c)
    after = perm()
    e.set_strata(None)
    dropped = perm()                                                 # nor does dropping the strata touch them
    e.close()
    assert np.array_equal(tab, c["tables"])
    for got in (after, dropped):
        assert np.array_equal(before[0], got[0]) and np.array_equal(_bytes(before[1]), _bytes(got[1]))
    assert before[0].any() and before[1].any()


def test_batch_and_text_calls_equal_the_device_call():
    c = cg.case((37, 45), 17, 20)
    e = cg.engine(c)
    dev, dev_tab = cg.run_dev(e, c)
    out, tab = e.assoc_cmh(c["codes"], c["is_x"], tables=True)
    assert np.array_equal(_bytes(out), _bytes(dev)) and np.array_equal(tab, dev_tab)
    # the text: rows on chromosome 7 and on X as the tokenizer flags them, a header line and a damaged line among them
    lines = [cg.text_of(c["codes"][v:v + 1], "X" if c["is_x"][v] else "7").replace(b"\t100\t", b"\t%d\t" % (100 + v)) for v in range(c["nv"])]
    text = b"".join(lines[:5]) + b"##a header line\n" + b"".join(lines[5:11]) + b"7\t55\n" + b"".join(lines[11:])
    HEADER, DAMAGED = 5, 12
    mark = np.zeros(c["nv"] + 3, hpgv.CMH_RESULT)                    # (a line per newline and one more: the wrapper's max_lines)
    mark["chisq"], mark["n_strata_bd"] = -7.0, -7
    res = e.assoc_cmh_text(text, tables=True, out=mark.copy())
    mark = mark[:c["nv"] + 2]
    e.close()
    assert res["n_lines"] == c["nv"] + 2
    st = res["status"]
    assert (st[HEADER] & 0xFF) != 0 and (st[DAMAGED] & 0xFF) != 0
    rec = np.ones(c["nv"] + 2, bool)
    rec[[HEADER, DAMAGED]] = False
    assert not (st[rec] & 0xFF).any()
    assert np.array_equal(_bytes(res["out"][rec]), _bytes(dev)) and np.array_equal(res["tables"][rec], dev_tab)
    assert np.array_equal(_bytes(res["out"][~rec]), _bytes(mark[~rec])) and not res["tables"][~rec].any()      # skipped: status set, record untouched


def test_a_group_context_deals_the_call():
    c = cg.case((37, 45), 17, 20)
    e = cg.engine(c)
    want = e.assoc_cmh(c["codes"], c["is_x"])
    e.close()
    g = cg.engine(c, device=[0, 0])
    for _ in range(3):                                               # both members take a call
        assert np.array_equal(_bytes(g.assoc_cmh(c["codes"], c["is_x"])), _bytes(want))
    g.close()
