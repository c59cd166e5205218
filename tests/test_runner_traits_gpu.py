"""What the file runners take from the tools' traits table (hpgv_host_internal.h: tool_of), seen from outside: which entries refuse
a run without a PED and with which words; the per-line arrays of a batch rebuilt at every width the table knows (4 ints and 3
doubles, 8 and 10, 4 and 6) when a batch holds more lines than it had room for; and the inheritance filter under a tool that installs no
assoc cohort and under one that installs its own."""
import ctypes as C
import os
from importlib import import_module

import numpy as np
import pytest

from helpers import hpgv
from test_record_filters_gpu import _key, _set, cohort, keep_of      # noqa: F401  (cohort: the fixture)
from test_record_filters_cpu import _RecFilters

pytestmark = pytest.mark.gpu

NEEDS_PED = b"this runner needs a PED file (ped_path is NULL)"
THREE_PATHS = b"vcf_path, ped_path and out_path must not be NULL"
LP = C.POINTER(C.c_long)


@pytest.fixture(scope="module")
def host():
    hpgv.build()
    L = C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)
    s, z, i, u64 = C.c_char_p, C.c_size_t, C.c_int, C.c_uint64
    L.hpgv_run_assoc.argtypes = [s, s, s, i, z, LP]
    L.hpgv_run_assoc_perm.argtypes = [s, s, s, i, u64, z, LP]
    L.hpgv_run_assoc_clump.argtypes = [s, s, s, i, C.c_void_p, z, LP, LP, LP]
    L.hpgv_run_assoc_model.argtypes = [s, s, s, i, u64, z, LP]
    L.hpgv_run_assoc_logistic.argtypes = [s, s, s, i, s, z, LP, LP]
    L.hpgv_run_assoc_linear.argtypes = [s, s, s, s, i, s, z, LP, LP]
    L.hpgv_run_tdt.argtypes = [s, s, s, z, LP]
    L.hpgv_run_tdt_perm.argtypes = [s, s, s, i, u64, z, LP]
    L.hpgv_run_vcf2epi.argtypes = [s, s, s, z, LP]
    L.hpgv_run_set_filters.argtypes = [C.c_void_p]
    L.hpgv_run_set_record_filters.argtypes = [C.POINTER(_RecFilters)]
    L.hpgv_host_last_error.restype = C.c_char_p
    L.hpgv_run_set_filters(None)
    L.hpgv_run_set_record_filters(None)
    yield L
    L.hpgv_run_set_filters(None)
    L.hpgv_run_set_record_filters(None)
    L.hpgv_host_shutdown()


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """60 samples in 15 families of two parents and two children, 20 records on one chromosome; a covariate file of three columns
    that lacks two samples and has one value that is no number; a phenotype file.  The same records once more behind 3 000 damaged
    lines of five bytes."""
    tmp = tmp_path_factory.mktemp("traits")
    rng = np.random.default_rng(31)
    people = []
    for f in range(15):
        fa, mo = "F%dp" % f, "F%dm" % f
        people += [("fam%d" % f, fa, "0", "0", 1, int(rng.integers(1, 3))), ("fam%d" % f, mo, "0", "0", 2, int(rng.integers(1, 3)))]
        people += [("fam%d" % f, "F%dc%d" % (f, k), fa, mo, int(rng.integers(1, 3)), 2 if k == 0 else int(rng.integers(1, 3))) for k in range(2)]
    names = [people[k][1] for k in rng.permutation(len(people))]
    assert len(names) == 60
    (tmp / "ped.txt").write_text("".join("%s %s %s %s %d %d\n" % p for p in people))
    fid = {p[1]: p[0] for p in people}
    cov_lines = ["FID IID AGE PC1 PC2\n"]
    for k, nm in enumerate(names):
        if k in (7, 41):
            continue
        cov_lines.append("%s %s %s %.4f %.4f\n" % (fid[nm], nm, "NA" if k == 19 else "%d" % rng.integers(20, 70), rng.normal(), rng.normal()))
    (tmp / "covar.txt").write_text("".join(cov_lines))
    (tmp / "pheno.txt").write_text("".join("%s %s %.5f\n" % (fid[nm], nm, rng.normal(10.0, 2.0)) for k, nm in enumerate(names) if k != 3))
    header = ("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n").encode()
    recs = []
    for v in range(20):
        gts = rng.choice(["0/0", "0/1", "1/1", "./."], size=60, p=[0.45, 0.35, 0.15, 0.05])
        recs.append(("1\t%d\trs%d\tA\tC\t50\tPASS\t.\tGT\t%s\n" % (1000 + 10 * v, v, "\t".join(gts))).encode())
    (tmp / "clean.vcf").write_bytes(header + b"".join(recs))
    (tmp / "damaged.vcf").write_bytes(header + b"1\t5\n" * 3000 + b"".join(recs))
    p = {k: str(tmp / k).encode() for k in ("ped.txt", "covar.txt", "pheno.txt", "clean.vcf", "damaged.vcf")}
    return dict(tmp=tmp, **p)


def _entries(L, c, vcf, ped, out, batch=1 << 22):
    """every public runner whose tool's row says needs_ped, by name: a call that returns (status, variants written)"""
    n, a, b = C.c_long(-1), C.c_long(-1), C.c_long(-1)
    opt = hpgv.RunClumpOptions()
    return {
        "assoc_chisq": lambda: (L.hpgv_run_assoc(vcf, ped, out, hpgv.TASK_CHISQ, batch, C.byref(n)), n.value),
        "assoc_fisher": lambda: (L.hpgv_run_assoc(vcf, ped, out, hpgv.TASK_FISHER, batch, C.byref(n)), n.value),
        "assoc_perm": lambda: (L.hpgv_run_assoc_perm(vcf, ped, out, 3, 5, batch, C.byref(n)), n.value),
        "assoc_clump": lambda: (L.hpgv_run_assoc_clump(vcf, ped, out, hpgv.TASK_CHISQ, C.addressof(opt), batch, C.byref(n), C.byref(a), C.byref(b)), n.value),
        "model": lambda: (L.hpgv_run_assoc_model(vcf, ped, out, 0, 0, batch, C.byref(n)), n.value),
        "model_perm": lambda: (L.hpgv_run_assoc_model(vcf, ped, out, 3, 5, batch, C.byref(n)), n.value),
        "logistic": lambda: (L.hpgv_run_assoc_logistic(vcf, ped, c["covar.txt"], 3, out, batch, C.byref(n), C.byref(a)), n.value),
        "tdt": lambda: (L.hpgv_run_tdt(vcf, ped, out, batch, C.byref(n)), n.value),
        "tdt_perm": lambda: (L.hpgv_run_tdt_perm(vcf, ped, out, 3, 5, batch, C.byref(n)), n.value),
        "vcf2epi": lambda: (L.hpgv_run_vcf2epi(vcf, ped, out, batch, C.byref(n)), n.value),
    }


NO_PED_MESSAGE = {
    "assoc_chisq": NEEDS_PED, "assoc_fisher": NEEDS_PED, "tdt": NEEDS_PED, "vcf2epi": NEEDS_PED,      # no argument check of their own
    "assoc_perm": THREE_PATHS, "model": THREE_PATHS, "model_perm": THREE_PATHS, "logistic": THREE_PATHS, "tdt_perm": THREE_PATHS,
    "assoc_clump": b"vcf_path, ped_path, out_path and the options must not be NULL",
}


@pytest.mark.parametrize("entry", list(NO_PED_MESSAGE))
def test_a_tool_that_needs_a_ped_refuses_a_run_without_one(host, small, tmp_path, entry):
    out = tmp_path / "o"
    rc, _ = _entries(host, small, small["clean.vcf"], None, str(out).encode())[entry]()
    assert rc == hpgv.ERR_INVALID
    assert host.hpgv_host_last_error() == NO_PED_MESSAGE[entry]
    assert os.listdir(tmp_path) == []                                # no output file, no side output


def _linear(L, c, ped, pheno, out, vcf="clean.vcf", batch=1 << 22):
    n, used = C.c_long(-1), C.c_long(-1)
    rc = L.hpgv_run_assoc_linear(c[vcf], ped, pheno, c["covar.txt"], 3, str(out).encode(), batch, C.byref(n), C.byref(used))
    return rc, n.value, used.value


def test_linear_takes_its_trait_from_a_ped_or_from_a_phenotype_file(host, small, tmp_path):
    c = small
    both = _linear(host, c, c["ped.txt"], c["pheno.txt"], tmp_path / "both")
    assert both[0] == 0, host.hpgv_host_last_error()
    assert both[1] == 20 and both[2] == 60 - 4                       # samples 7, 41 (no covariate line), 19 (NA), 3 (no trait)
    assert _linear(host, c, None, c["pheno.txt"], tmp_path / "pheno") == both
    assert (tmp_path / "pheno").read_bytes() == (tmp_path / "both").read_bytes()
    assert len((tmp_path / "both").read_bytes().splitlines()) == 21
    rc, n, used = _linear(host, c, None, None, tmp_path / "neither")
    assert rc == hpgv.ERR_INVALID and (n, used) == (0, 0)
    assert host.hpgv_host_last_error() == b"the trait needs a PED file or a phenotype file (ped_path and pheno_path are NULL)"
    assert not (tmp_path / "neither").exists()


@pytest.mark.parametrize("entry", ["assoc_chisq", "tdt", "model", "logistic", "linear"])
def test_batch_arrays_are_rebuilt_at_every_width(host, small, tmp_path, entry):
    # 3 000 damaged lines "1\t5\n" in front of the records, in a 64 KiB batch sized for 65536 / (2 * 60 + 18) + 2 = 476 lines: the
    # engine reports 3 020, the arrays are rebuilt at the tool's width and the batch is done again.  A damaged line has no ALT
    # field and gives no record, so the file is the one of the records alone
    c = small
    got = {}
    for vcf in ("clean.vcf", "damaged.vcf"):
        out = tmp_path / (vcf + ".out")
        if entry == "linear":
            rc, n, _ = _linear(host, c, c["ped.txt"], c["pheno.txt"], out, vcf, 1 << 16)
        else:
            rc, n = _entries(host, c, c[vcf], c["ped.txt"], str(out).encode(), 1 << 16)[entry]()
        assert rc == 0, host.hpgv_host_last_error()
        got[vcf] = (n, out.read_bytes())
    assert got["clean.vcf"][0] == 20 and len(got["clean.vcf"][1].splitlines()) == 21
    assert got["damaged.vcf"] == got["clean.vcf"]


def _body(path):
    lines = open(path, "rb").read().splitlines(keepends=True)
    return [l for l in lines if l.startswith(b"#")], [l for l in lines if not l.startswith(b"#")]


def test_inheritance_filter_scans_the_cohort_of_the_tool_or_of_the_ped(host, cohort, tmp_path):
    # the logistic run installs its own assoc cohort -- the PED's cases and controls less the samples without covariates -- and
    # --inh-dom scans that one; the TDT run, right after it, installs none and gets the PED's.  Each filtered file is the
    # unfiltered one restricted to the records the definition keeps for that cohort
    c = cohort
    names = c["header"].splitlines()[-1].decode().split("\t")[9:]
    rng = np.random.default_rng(5)
    with_cov = rng.random(len(names)) < 0.6
    (tmp_path / "covar.txt").write_text("".join("x %s %.4f\n" % (nm, rng.normal()) for nm, w in zip(names, with_cov) if w))
    cond_cov = np.where(with_cov, c["cond"], hpgv.COND_OTHER).astype(np.uint8)
    vcf, ped, cov = c["paths"]["plain"].encode(), c["ped"].encode(), str(tmp_path / "covar.txt").encode()
    n, used = C.c_long(-1), C.c_long(-1)

    def runs(tag):
        r1 = host.hpgv_run_assoc_logistic(vcf, ped, cov, 1, str(tmp_path / (tag + ".logistic")).encode(), 1 << 18, C.byref(n), C.byref(used))
        n_log = n.value
        r2 = host.hpgv_run_tdt(vcf, ped, str(tmp_path / (tag + ".tdt")).encode(), 1 << 18, C.byref(n))
        return r1, r2, n_log, n.value

    host.hpgv_run_set_record_filters(None)
    assert runs("all")[:2] == (0, 0), host.hpgv_host_last_error()
    assert used.value == int(((cond_cov == hpgv.COND_AFFECTED) | (cond_cov == hpgv.COND_UNAFFECTED)).sum())
    R = _set(host, c, dict(min_dominant=0.6))
    host.hpgv_run_set_filters(None)
    try:
        r1, r2, n_log, n_tdt = runs("some")
    finally:
        host.hpgv_run_set_record_filters(None)
    assert (r1, r2) == (0, 0), host.hpgv_host_last_error()
    keep_ped, keep_cov = keep_of(c, R), keep_of(dict(c, cond=cond_cov), R)
    assert 0 < keep_ped.sum() < len(keep_ped) and 0 < keep_cov.sum() < len(keep_cov)
    assert (keep_ped != keep_cov).sum() >= 20                        # the two cohorts keep different records: a swap would show
    for suffix, keep, count in ((".logistic", keep_cov, n_log), (".tdt", keep_ped, n_tdt)):
        kept = {(r["chrom"].encode(), r["pos"]) for r, k in zip(c["recs"], keep) if k}
        head, body = _body(tmp_path / ("all" + suffix))
        assert len(body) == len(keep)
        assert open(tmp_path / ("some" + suffix), "rb").read() == b"".join(head + [l for l in body if _key(l) in kept]), suffix
        assert count == int(keep.sum())
