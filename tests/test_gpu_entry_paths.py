"""The batch and text entry points share one back half per tool (hpgv_tool_capi.hip; the text's front half is in
hpgv_text_capi.hip).  Two things no other test pins:
the clamp of the multi-allelic tables to the caller's capacity -- one function behind hpgv_stats_ex and
hpgv_stats_text_groups, fused and as a kernel chain -- and the bad-argument codes of the entry points that are now
guarded against C++ exceptions."""
import ctypes as C

import numpy as np
import pytest

from helpers import hpgv

pytestmark = pytest.mark.gpu


def _text(codes):
    names = np.array([str(i) for i in range(15)] + ["."])
    cells = np.char.add(np.char.add(names[codes >> 4], "/"), names[codes & 15])
    return "".join("7\t%d\trs%d\tA\tC,G\t.\tPASS\t.\tGT\t%s\n" % (100 + v, v, "\t".join(cells[v]))
                   for v in range(codes.shape[0])).encode()


def _stats_text(e, text, m, cap, n_samples, with_missing):
    p = lambda a: C.c_void_p(a.ctypes.data)
    nl, nm = C.c_int(0), C.c_int(cap)
    line_off, field_off, status = np.zeros(m + 2, np.uint64), np.zeros(m * 10, np.uint32), np.zeros(m, np.int32)
    c8, hw, sm = np.zeros(m * 8, np.int32), np.zeros(2 * m), np.zeros(n_samples, np.int32)
    midx, mtab = np.full(m, -1, np.int32), np.full((m, 256), -1, np.int32)
    rc = e.L.hpgv_stats_text_groups(e.h, text, len(text), m, C.byref(nl), p(line_off), p(field_off), p(status), p(c8), p(hw), p(hw[m:]),
                                    p(sm) if with_missing else None, p(midx), p(mtab), C.byref(nm), None, None, None, None, None)
    assert rc == 0, e.L.hpgv_last_error(e.h)
    assert nl.value == m
    return dict(n_multi=nm.value, multi_idx=midx, multi_table=mtab)


def test_multi_allelic_tables_clamp_to_the_capacity_on_batch_and_text():
    for n_samples in (37, 1000):
        _check_clamp(n_samples)


def _check_clamp(n_samples):
    rng = np.random.default_rng(n_samples)
    m, cap = 90, 5
    # fully called or fully missing genotypes only: a variant is multi-allelic exactly when it holds allele 2
    codes = rng.choice(np.array([0x00, 0x01, 0x10, 0x11, 0xFF], np.uint8), size=(m, n_samples), p=[0.5, 0.15, 0.15, 0.15, 0.05])
    multi = np.sort(rng.choice(m, 17, replace=False))
    for v in multi:
        codes[v, rng.choice(n_samples, 3, replace=False)] = (0x12, 0x22, 0x20)
    exp_idx = multi[:cap].astype(np.int32)
    exp_tab = np.stack([np.bincount(codes[v], minlength=256) for v in exp_idx]).astype(np.int32)
    text = _text(codes)
    e = hpgv.Engine(0)
    e.set_stats_cohort(n_samples)
    for fused in (1, 0):
        e.set_option("batch_fused", fused)
        for with_missing in (False, True):       # a batch: without per-sample counters the per-batch kernel, with them k_stats_all
            acc = np.zeros(n_samples, np.int32) if with_missing else None
            b = e.stats_ex(codes, sample_missing=acc, multi_cap=cap)
            assert b["n_multi"] == len(multi)                                   # how many there are, not how many fit
            assert np.array_equal(b["multi_idx"], exp_idx)
            assert np.array_equal(b["multi_table"], exp_tab)
            t = _stats_text(e, text, m, cap, n_samples, with_missing)
            assert t["n_multi"] == len(multi)
            assert np.array_equal(t["multi_idx"][:cap], exp_idx)
            assert np.array_equal(t["multi_table"][:cap], exp_tab)
            assert (t["multi_idx"][cap:] == -1).all() and (t["multi_table"][cap:] == -1).all()   # nothing behind the capacity
        z = e.stats_ex(codes, multi_cap=0)                                      # no room at all: the count alone
        assert z["n_multi"] == len(multi) and len(z["multi_idx"]) == 0
    e.close()


def test_guarded_entry_points_still_refuse_bad_arguments():
    n_samples, nv = 20, 4
    e = hpgv.Engine(0)
    L = e.L
    e.set_cohort((np.arange(n_samples) % 2).astype(np.uint8))
    e.set_stats_cohort(n_samples)
    e.set_stats_groups((np.arange(n_samples) % 2).astype(np.int32), 2)
    gt = np.zeros((nv, n_samples), np.uint8)
    i4 = [np.zeros(nv, np.int32) for _ in range(4)]
    f3 = [np.zeros(nv) for _ in range(3)]
    c8, hw = np.zeros(2 * nv * 8, np.int32), np.zeros(2 * nv)
    out = np.zeros((nv, n_samples), np.uint8)
    text = _text(gt)
    nl = C.c_int(0)
    p = lambda a: C.c_void_p(a.ctypes.data)
    ints, dbls = [p(a) for a in i4], [p(a) for a in f3]
    bad = [
        L.hpgv_assoc(e.h, 7, p(gt), n_samples, nv, None, *ints, *dbls),                                  # no such task
        L.hpgv_assoc(e.h, hpgv.TASK_CHISQ, None, n_samples, nv, None, *ints, *dbls),                     # no batch
        L.hpgv_assoc(e.h, hpgv.TASK_CHISQ, p(gt), n_samples, nv, None, *ints, dbls[0], None, dbls[2]),   # chi-square without its output
        L.hpgv_assoc(e.h, hpgv.TASK_CHISQ, p(gt), n_samples - 1, nv, None, *ints, *dbls),                # rows shorter than the cohort
        L.hpgv_assoc_text(e.h, 7, text, len(text), nv, C.byref(nl), None, None, None, *ints, *dbls),
        L.hpgv_assoc_text(e.h, hpgv.TASK_CHISQ, text, len(text), nv, None, None, None, None, *ints, *dbls),   # n_lines is NULL
        L.hpgv_assoc_text(e.h, hpgv.TASK_CHISQ, text, len(text), -1, C.byref(nl), None, None, None, *ints, *dbls),
        L.hpgv_stats_groups(e.h, None, n_samples, nv, p(c8), None, None),
        L.hpgv_stats_groups(e.h, p(gt), n_samples, nv, p(c8), p(hw), None),                              # hwe_chi2 without hwe_p
        L.hpgv_stats_groups(e.h, p(gt), n_samples - 1, nv, p(c8), None, None),
        L.hpgv_epi_dataset(e.h, p(gt), n_samples, nv, None),
        L.hpgv_epi_dataset(e.h, p(gt), n_samples, -1, p(out)),
        L.hpgv_epi_dataset(e.h, p(gt), n_samples - 1, nv, p(out)),
        L.hpgv_epi_dataset_text(e.h, text, len(text), nv, C.byref(nl), None, None, None, None),          # no output rows
        L.hpgv_epi_dataset_text(e.h, text, len(text), nv, None, None, None, None, p(out)),
    ]
    assert bad == [hpgv.ERR_INVALID] * len(bad)
    # and the same calls with good arguments go through
    assert L.hpgv_assoc(e.h, hpgv.TASK_CHISQ, p(gt), n_samples, nv, None, *ints, *dbls) == hpgv.OK
    assert L.hpgv_assoc_text(e.h, hpgv.TASK_CHISQ, text, len(text), nv, C.byref(nl), None, None, None, *ints, *dbls) == hpgv.OK and nl.value == nv
    assert L.hpgv_stats_groups(e.h, p(gt), n_samples, nv, p(c8), None, None) == hpgv.OK
    assert L.hpgv_epi_dataset(e.h, p(gt), n_samples, nv, p(out)) == hpgv.OK
    assert L.hpgv_epi_dataset_text(e.h, text, len(text), nv, C.byref(nl), None, None, None, p(out)) == hpgv.OK and nl.value == nv
    e.close()
