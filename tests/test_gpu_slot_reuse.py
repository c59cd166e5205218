"""One slot, many tools.  Every synchronous entry point leases a per-call slot of grow-only device buffers (Slot,
hpgv_internal.h), and with one thread every call gets the same one: a buffer a call finds may have been left by any other
tool, larger or smaller than it needs.  Case 1 runs every tool in turn on one engine with everything set -- cohort, stats
cohort, groups, pedigree, families, log-factorials, all record filters -- at 8, then 300, then 8 lines, with the one-pass
kernels and with the kernel chain, and wants every output bit for bit what the same call gives on a fresh engine of its
own, whose buffers no other call has used.  Every output is bit-reproducible between fresh engines, on the commit before
the named slot buffers too: none is compared with a tolerance.  At 37 samples the pedigree has 40 trios over those
columns, which hpgv_mendel_layout allows: its row is longer than the stats row (asserted below), so the chain's re-layout
for the Mendelian errors grows the laid-out buffer in mid-call; at 1 000 samples the 8-to-300 step does.  Case 2: a text
held by hpgv_filter_text keeps its slot while other calls run on another."""
import ctypes as C
import gzip

import numpy as np
import pytest

from helpers import assert_close, check_assoc, hpgv, make_families, oracle_assoc
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

LINE_FILTERED = 0x100                                          # include/hpgv.h HPGV_LINE_FILTERED
CODES = np.array([0x00, 0x01, 0x10, 0x11, 0xFF, 0x0F, 0x12, 0x22], np.uint8)
CODE_P = [0.34, 0.2, 0.2, 0.2, 0.02, 0.02, 0.01, 0.01]
MULTI_CAP = 5
LINE_COUNTS = (8, 300, 8)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _argtypes(L):
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    L.hpgv_filter_text.argtypes = [vp, vp, sz, i32, C.POINTER(i32), vp, vp, vp]
    L.hpgv_text_partition.argtypes = [vp, vp, vp, i32, vp, sz, vp, vp]
    L.hpgv_text_multisplit.argtypes = [vp, vp, vp, i32, i32, i32, vp, sz, vp]


def _text(codes, chroms):
    names = np.array([str(i) for i in range(15)] + ["."])
    cells = np.char.add(np.char.add(names[codes >> 4], "/"), names[codes & 15])
    return "".join("%s\t%d\trs%d\tA\tC,G\t.\tPASS\t.\tGT\t%s\n" % (chroms[v], 100 + v, v, "\t".join(cells[v]))
                   for v in range(codes.shape[0])).encode()


def _cohort(n_samples):
    rng = np.random.default_rng(1000 + n_samples)
    c = dict(n_samples=n_samples)
    c["cond"] = rng.choice([0, 1, 2], size=n_samples, p=[0.45, 0.45, 0.1]).astype(np.uint8)
    c["groups"] = rng.integers(0, 2, n_samples).astype(np.int32)
    n_trios = 40 if n_samples < 100 else n_samples // 3
    trios = np.array([rng.choice(n_samples, 3, replace=False) for _ in range(n_trios)], np.int32)
    c["trios"] = (trios[:, 0].copy(), trios[:, 1].copy(), trios[:, 2].copy(), rng.integers(0, 2, n_trios).astype(np.uint8))
    c["families"] = make_families(rng, n_samples, n_samples // 4, 3, p_absent=0.03)
    c["lf"] = orc.logfact(n_samples * 10)
    return c


def _lines(n_samples, n_lines):
    """codes as the tokenizer gives them (half-called genotypes kept); every fourth row has seven missing genotypes in ten: the
    count filters reject it"""
    rng = np.random.default_rng(7 * n_samples + n_lines)
    codes = CODES[rng.choice(len(CODES), size=(n_lines, n_samples), p=CODE_P)]
    codes[::4, :-(-7 * n_samples // 10)] = 0xFF
    chroms = np.where(rng.random(n_lines) < 0.3, "X", "7")
    strict = np.where(((codes >> 4) == 0xF) | ((codes & 0xF) == 0xF), 0xFF, codes).astype(np.uint8)
    return dict(codes=codes, strict=strict, is_x=(chroms == "X").astype(np.uint8), text=_text(codes, chroms), n=n_lines)


def _engine(c):
    e = hpgv.Engine(0)
    _argtypes(e.L)
    n = c["n_samples"]
    e.set_cohort(c["cond"])
    e.set_stats_cohort(n)
    e.set_stats_groups(c["groups"], 2)
    e.set_pedigree(n, *c["trios"])
    e.set_families(n, *c["families"])
    e.set_logfact(c["lf"])
    assert e.L.hpgv_set_text_filters(e.h, C.c_double(0.05), C.c_double(0.5), C.c_long(len(c["trios"][0]))) == 0
    e.set_text_inheritance_filters(0.3, 0.3)
    return e


def _stats_text(e, c, d):
    L, m, ns, nt = e.L, d["n"], c["n_samples"], len(c["trios"][0])
    nl, nm = C.c_int(0), C.c_int(MULTI_CAP)
    o = dict(line_off=np.zeros(m + 2, np.uint64), field_off=np.zeros(m * 10, np.uint32), status=np.zeros(m, np.int32),
             c8=np.zeros((m, 8), np.int32), chi2=np.zeros(m), p=np.zeros(m), smiss=np.zeros(ns, np.int32),
             midx=np.full(MULTI_CAP, -1, np.int32), mtab=np.full((MULTI_CAP, 256), -1, np.int32), merr=np.zeros(m, np.int32),
             cerr=np.zeros(nt, np.int32), gc8=np.zeros((2, m, 8), np.int32), gchi2=np.zeros((2, m)), gp=np.zeros((2, m)))
    rc = L.hpgv_stats_text_groups(e.h, d["text"], len(d["text"]), m, C.byref(nl), _p(o["line_off"]), _p(o["field_off"]), _p(o["status"]),
                                  _p(o["c8"]), _p(o["chi2"]), _p(o["p"]), _p(o["smiss"]), _p(o["midx"]), _p(o["mtab"]), C.byref(nm),
                                  _p(o["merr"]), _p(o["cerr"]), _p(o["gc8"]), _p(o["gchi2"]), _p(o["gp"]))
    assert rc == 0, L.hpgv_last_error(e.h)
    assert nl.value == m
    o["n_multi"] = np.array([nm.value])
    return o


def _hold(e, buf, m):
    L = e.L
    nl = C.c_int(0)
    lo, fo, st = np.zeros(m + 1, np.uint64), np.zeros(10 * m, np.uint32), np.zeros(m, np.int32)
    assert L.hpgv_filter_text(e.h, buf.ctypes.data, buf.nbytes, m, C.byref(nl), _p(lo), _p(fo), _p(st)) == 0, L.hpgv_last_error(e.h)
    assert nl.value == m
    return dict(line_off=lo, field_off=fo, status=st)


def _partition(e, buf, keep, m):
    out = np.zeros(buf.nbytes, np.uint8)
    kb, tb = C.c_uint64(0), C.c_uint64(0)
    assert e.L.hpgv_text_partition(e.h, buf.ctypes.data, _p(keep), m, _p(out), out.nbytes, C.byref(kb), C.byref(tb)) == 0, e.L.hpgv_last_error(e.h)
    assert tb.value == buf.nbytes
    return out[:kb.value].tobytes(), out[kb.value:tb.value].tobytes()


def _gunzip(members):
    return gzip.decompress(members) if members else b""


def _steps(c, d):
    """every tool once on the lines `d`, as steps f(engine) -> {call: {output: array or bytes}}.  A step is one call, or the calls
    that need each other: hpgv_filter_text and the line tool that runs on the text it holds"""
    m, ns = d["n"], c["n_samples"]
    text = d["text"]
    buf = np.frombuffer(text, np.uint8).copy()
    bucket = (np.arange(m) % 3).astype(np.uint8)

    def epi_text(e):
        nA, nU, _ = e.assoc_layout()
        nl, epi, st = C.c_int(0), np.zeros((m, nA + nU), np.uint8), np.zeros(m, np.int32)
        assert e.L.hpgv_epi_dataset_text(e.h, text, len(text), m, C.byref(nl), None, None, _p(st), _p(epi)) == 0, e.L.hpgv_last_error(e.h)
        assert nl.value == m
        return dict(rows=epi, status=st)

    def stats_ex(e):
        smiss = np.zeros(ns, np.int32)
        return dict(e.stats_ex(d["codes"], sample_missing=smiss, multi_cap=MULTI_CAP), smiss=smiss)

    def mendel(e):
        cerr = np.zeros(len(c["trios"][0]), np.int32)
        return dict(errors=e.mendel(d["codes"], d["is_x"], child_errors=cerr), child_errors=cerr)

    def held(e, tag):
        h = _hold(e, buf, m)
        return {"filter_text" + tag: h}, ((h["status"] & LINE_FILTERED) == 0).astype(np.uint8)

    def partition(e):
        r, keep = held(e, "")
        kept, rest = _partition(e, buf, keep, m)
        return dict(r, partition=dict(kept=kept, rest=rest))

    def partition_bgzf(e):
        r, keep = held(e, "_2")
        cap = e.L.hpgv_bgzf_deflate_bound(buf.nbytes, 2)
        out, comp, last = np.zeros(cap, np.uint8), (C.c_uint64 * 2)(), (C.c_uint8 * 2)()
        kb, tb = C.c_uint64(0), C.c_uint64(0)
        assert e.L.hpgv_text_partition_bgzf(e.h, buf.ctypes.data, _p(keep), m, _p(out), cap, 1, C.byref(kb), C.byref(tb), comp, last) == 0, e.L.hpgv_last_error(e.h)
        return dict(r, partition_bgzf=dict(kept=_gunzip(out[:comp[0]].tobytes()), rest=_gunzip(out[comp[0]:comp[0] + comp[1]].tobytes()),
                                           sizes=np.array([kb.value, tb.value]), last=bytes(last)))

    def multisplit(e):
        r, _ = held(e, "_3")
        for name, first, cnt in (("multisplit_a", 0, m // 2), ("multisplit_b", m // 2, m - m // 2)):
            out, boff = np.zeros(buf.nbytes, np.uint8), np.zeros(4, np.uint64)
            assert e.L.hpgv_text_multisplit(e.h, buf.ctypes.data, _p(bucket[first:]), first, cnt, 3, _p(out), out.nbytes, _p(boff)) == 0, e.L.hpgv_last_error(e.h)
            r[name] = dict(lines=out[:int(boff[3])].tobytes(), bucket_off=boff)
        assert e.L.hpgv_text_partition(e.h, buf.ctypes.data, None, 0, None, 0, None, None) == 0      # the hold released
        return r

    def compress(e):
        cap = e.L.hpgv_bgzf_deflate_bound(buf.nbytes, 1)
        out, made = np.zeros(cap, np.uint8), C.c_size_t(0)
        assert e.L.hpgv_bgzf_compress(e.h, buf.ctypes.data, buf.nbytes, _p(out), cap, C.byref(made)) == 0, e.L.hpgv_last_error(e.h)
        return dict(bgzf_compress=dict(text=_gunzip(out[:made.value].tobytes())))

    one = lambda name, f: (lambda e: {name: f(e)})
    return [one("tokenize", lambda e: e.tokenize(text, ns, strict=False, max_lines=m)),
            one("assoc_text_chisq", lambda e: e.assoc_text(hpgv.TASK_CHISQ, text, m)),
            one("assoc_text_fisher", lambda e: e.assoc_text(hpgv.TASK_FISHER, text, m)),
            one("tdt_text", lambda e: e.tdt_text(text, m)),
            one("stats_text", lambda e: _stats_text(e, c, d)),
            one("epi_text", epi_text),
            one("assoc_chisq", lambda e: e.assoc(hpgv.TASK_CHISQ, d["strict"], d["is_x"])),
            one("assoc_fisher", lambda e: e.assoc(hpgv.TASK_FISHER, d["strict"], d["is_x"])),
            one("stats_ex", stats_ex), one("mendel", mendel), partition, partition_bgzf, multisplit, compress]


def _sequence(e, c, d):
    """all steps in turn on the one engine `e`"""
    r = {}
    for step in _steps(c, d):
        r.update(step(e))
    return r


def _reference(c, d, fused):
    """every step on a fresh engine of its own: buffers that no other call has used"""
    r = {}
    for step in _steps(c, d):
        f = _engine(c)
        f.set_option("batch_fused", fused)
        r.update(step(f))
        f.close()
    return r


def _same(got, exp, where):
    assert got.keys() == exp.keys(), where
    for call in exp:
        for k, x in exp[call].items():
            y = got[call][k]
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (where, call, k)
            else:
                assert x == y, (where, call, k)


def _against_the_oracle(c, d, r):
    lines = d["text"].splitlines(keepends=True)
    status = r["filter_text"]["status"]
    out = (status & LINE_FILTERED) != 0
    assert out[::4].all() and 0 < out.sum() < d["n"], "the filters reject some lines and keep others"
    for k in ("assoc_text_chisq", "assoc_text_fisher", "tdt_text", "stats_text", "epi_text"):
        assert np.array_equal(r[k]["status"], status), k             # the same verdicts from every text entry point
    assert np.array_equal(r["tokenize"]["gt"], d["codes"]) and np.array_equal(r["tokenize"]["is_x"], d["is_x"])
    for task, name in ((hpgv.TASK_CHISQ, "chisq"), (hpgv.TASK_FISHER, "fisher")):
        exp = oracle_assoc(task, d["strict"], c["cond"], d["is_x"], c["lf"])
        check_assoc(r["assoc_text_" + name], exp, task)
        check_assoc(r["assoc_" + name], exp, task)
    s, b = r["stats_text"], r["stats_ex"]
    for i in range(d["n"]):
        vs = orc.variant_stats(d["codes"][i], 2)
        for c8, chi2, p in ((s["c8"][i], s["chi2"][i], s["p"][i]), (b["counts8"][i], b["hwe_chi2"][i], b["hwe_p"][i])):
            assert list(c8[:4]) == list(vs.genotypes_count)[:4], i
            assert c8[4] == vs.missing_genotypes and c8[5] == vs.missing_alleles and c8[6] == vs.alleles_count[0] and c8[7] == vs.alleles_count[1], i
            assert_close([chi2], [vs.hw_chi2], "hwe chi2"); assert_close([p], [vs.hw_p], "hwe p")
        for g in range(2):
            gs = orc.variant_stats(np.ascontiguousarray(d["codes"][i][c["groups"] == g]), 2)
            assert list(s["gc8"][g, i, :4]) == list(gs.genotypes_count)[:4], (i, g)
            assert_close([s["gchi2"][g, i]], [gs.hw_chi2], "group hwe chi2"); assert_close([s["gp"][g, i]], [gs.hw_p], "group hwe p")
    assert np.array_equal(s["smiss"], orc.sample_missing(d["codes"])) and np.array_equal(b["smiss"], s["smiss"])
    err, trio = orc.mendel_counts(d["codes"], *c["trios"], d["is_x"])
    assert np.array_equal(s["merr"], err) and np.array_equal(s["cerr"], trio)
    assert np.array_equal(r["mendel"]["errors"], err) and np.array_equal(r["mendel"]["child_errors"], trio)
    multi = [i for i in range(d["n"]) if np.isin(d["codes"][i], (0x12, 0x22)).any()]
    assert s["n_multi"][0] == len(multi) and list(s["midx"][:min(len(multi), MULTI_CAP)]) == multi[:MULTI_CAP]
    # the line tools: the numpy partition of the lines, the bgzip twins equal to the plain ones
    assert r["partition"]["kept"] == b"".join(l for l, o in zip(lines, out) if not o)
    assert r["partition"]["rest"] == b"".join(l for l, o in zip(lines, out) if o)
    assert (r["partition_bgzf"]["kept"], r["partition_bgzf"]["rest"]) == (r["partition"]["kept"], r["partition"]["rest"])
    half = d["n"] // 2
    for name, part in (("multisplit_a", lines[:half]), ("multisplit_b", lines[half:])):
        first = 0 if name.endswith("a") else half
        assert r[name]["lines"] == b"".join(b"".join(l for j, l in enumerate(part) if (first + j) % 3 == k) for k in range(3)), name
    assert r["bgzf_compress"]["text"] == d["text"]


@pytest.mark.parametrize("n_samples", [37, 1000])
def test_one_slot_many_tools_growing_then_shrinking(n_samples):
    c = _cohort(n_samples)
    data = {n: _lines(n_samples, n) for n in set(LINE_COUNTS)}
    e = _engine(c)                                                  # one engine, one thread: every call leases the same slot
    if n_samples == 37:                                             # the Mendel row is the longer one: the chain grows `laid` in mid-call
        mendel, stats = C.c_size_t(0), C.c_size_t(0)
        assert e.L.hpgv_mendel_layout(e.h, C.byref(mendel)) == 0 and e.L.hpgv_stats_layout(e.h, C.byref(stats)) == 0
        assert mendel.value > stats.value
    fresh = {}
    for fused in (1, 0):
        e.set_option("batch_fused", fused)
        for n in LINE_COUNTS:
            if (fused, n) not in fresh:                             # the same calls, each on buffers that have never been used
                fresh[fused, n] = _reference(c, data[n], fused)
                _against_the_oracle(c, data[n], fresh[fused, n])
            _same(_sequence(e, c, data[n]), fresh[fused, n], (fused, n))
    e.close()


def test_a_hold_keeps_its_slot():
    c = _cohort(37)
    a, b = _lines(37, 300), _lines(37, 340)
    e = _engine(c)
    buf = np.frombuffer(a["text"], np.uint8).copy()
    held = _hold(e, buf, a["n"])                                    # text A stays on the device, in its slot
    got = dict(assoc=e.assoc_text(hpgv.TASK_CHISQ, b["text"], b["n"]), stats=_stats_text(e, c, b))      # another slot
    out = (held["status"] & LINE_FILTERED) != 0
    assert 0 < out.sum() < a["n"]
    kept, rest = _partition(e, buf, (~out).astype(np.uint8), a["n"])
    lines = a["text"].splitlines(keepends=True)
    assert kept == b"".join(l for l, o in zip(lines, out) if not o)
    assert rest == b"".join(l for l, o in zip(lines, out) if o)
    e.close()
    exp = {}
    for name, call in (("assoc", lambda f: f.assoc_text(hpgv.TASK_CHISQ, b["text"], b["n"])), ("stats", lambda f: _stats_text(f, c, b))):
        f = _engine(c)
        exp[name] = call(f)
        f.close()
    _same(got, exp, "text B")
