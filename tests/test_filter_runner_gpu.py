"""hpgv_run_filter (hpg-var-vcf filter, filter_runner.c:23-260): the records that pass the filter chain in <prefix>.filtered,
the others in <prefix>.rejected, byte for byte and in file order, the lines partitioned on the device.  The keep mask comes
from the oracle (as test_run_assoc_with_record_filters computes it); the same bytes from plain, gzip and bgzip input, from
small batches and from a group context on which a bgzip file is staged in parts."""
import ctypes as C
import gzip
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

from helpers import hpgv
from oracle import pyoracle as orc
from test_host_logic_cpu import _bgzf
from test_host_mirror_gpu import _write_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Filters(C.Structure):
    _fields_ = [("min_maf", C.c_double), ("max_missing", C.c_double), ("max_mendel_errors", C.c_int),
                ("num_alleles", C.c_int), ("min_quality", C.c_double)]


FILTERS = {"maf": _Filters(0.1, -1, -1, -1, -1), "missing": _Filters(-1, 0.1, -1, -1, -1), "mendel": _Filters(-1, -1, 1, -1, -1),
           "alleles": _Filters(-1, -1, -1, 2, -1), "quality": _Filters(-1, -1, -1, -1, 30.0), "all": _Filters(0.02, 0.4, 50, 2, 5.0)}


@pytest.fixture(scope="module")
def host():
    hpgv.build()
    L = C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)
    L.hpgv_run_filter.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.hpgv_run_set_filters.argtypes = [C.POINTER(_Filters)]
    L.hpgv_host_last_error.restype = C.c_char_p
    yield L
    L.hpgv_run_set_filters(None)
    L.hpgv_host_shutdown()


def _filter_lines(F):
    out = []
    if F.min_maf >= 0: out.append('##FILTER=<ID=maf,Description="Minor allele frequency >= %g">\n' % F.min_maf)
    if F.max_missing >= 0: out.append('##FILTER=<ID=missing,Description="Rate of missing genotypes <= %g">\n' % F.max_missing)
    if F.max_mendel_errors >= 0: out.append('##FILTER=<ID=mendel,Description="Mendelian errors <= %g">\n' % F.max_mendel_errors)
    if F.num_alleles >= 0: out.append('##FILTER=<ID=alleles,Description="Number of alleles == %g">\n' % F.num_alleles)
    if F.min_quality >= 0: out.append('##FILTER=<ID=quality,Description="Quality >= %g">\n' % F.min_quality)
    return "".join(out).encode()


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    """1 200 records of ~120 samples (~550 KB of text: more than 300 bgzip blocks of 0x700 bytes), with rare, missing-heavy,
    multi-allelic and low-quality records; the oracle's values of every filter per record"""
    tmp = tmp_path_factory.mktemp("filter")
    rng = np.random.default_rng(31)
    people, names, rows = _write_inputs(tmp, rng, 25, 20, 1200)
    n = len(names)
    alts, quals = [], []
    for v, (chrom, fmt, samples) in enumerate(rows):
        pos = fmt.split(":").index("GT")
        if v % 5 == 0:
            for k in range(n):
                if rng.random() < 0.9:
                    parts = samples[k].split(":"); parts[pos] = "0/0"; samples[k] = ":".join(parts)
        if v % 7 == 0:
            for k in range(n):
                if rng.random() < 0.3:
                    parts = samples[k].split(":"); parts[pos] = "./."; samples[k] = ":".join(parts)
        alts.append(["C", "C,G", ".", "C,G,T"][v % 4]); quals.append([".", "10", "35.5", "90"][v % 4 if v % 3 else 3])
    header = ("##fileformat=VCFv4.1\n##source=test\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n").encode()
    lines = [("%s\t%d\trs%d\tA\t%s\t%s\tPASS\t.\t%s\t%s\n" % (chrom, 1000 + v, v, alts[v], quals[v], fmt, "\t".join(samples))).encode()
             for v, (chrom, fmt, samples) in enumerate(rows)]
    lax = np.array([[orc.encode_sample(s, fmt.split(":").index("GT"), False) for s in samples] for _, fmt, samples in rows], np.uint8)
    is_x = np.array([1 if c == "X" else 0 for c, _, _ in rows], np.uint8)
    col = {nm: i for i, nm in enumerate(names)}
    trios = [(col[p[2]], col[p[3]], col[p[1]], orc.MALE if p[4] == 1 else orc.FEMALE) for p in people
             if p[2] != "0" and p[3] != "0" and p[1] in col and p[2] in col and p[3] in col]
    merr, _ = orc.mendel_counts(lax, [t[0] for t in trios], [t[1] for t in trios], [t[2] for t in trios], [t[3] for t in trios], is_x)
    maf, miss = np.zeros(len(rows)), np.zeros(len(rows))
    for v in range(len(rows)):
        vs = orc.variant_stats(lax[v], 2)
        a0, a1 = vs.alleles_count[0], vs.alleles_count[1]
        maf[v] = min(a0, a1) / (a0 + a1) if a0 + a1 else 0.0
        miss[v] = vs.missing_genotypes / n
    n_alleles = np.array([1 if a == "." else 1 + len(a.split(",")) for a in alts])
    qual = np.array([-1.0 if q == "." else float(q) for q in quals])
    data = header + b"".join(lines)
    paths = {"plain": tmp / "in.vcf", "gzip": tmp / "in.vcf.gzip.gz", "bgzip": tmp / "in.vcf.gz"}
    paths["plain"].write_bytes(data)
    paths["gzip"].write_bytes(gzip.compress(data, 6))
    packed = _bgzf(data, 0x700)
    paths["bgzip"].write_bytes(packed)
    assert len(data) // 0x700 >= 300
    return dict(tmp=tmp, header=header, lines=lines, ped=str(tmp / "ped.txt"), paths={k: str(v) for k, v in paths.items()},
                merr=merr, maf=maf, miss=miss, n_alleles=n_alleles, qual=qual)


def _keep(c, F):
    keep = np.ones(len(c["lines"]), bool)
    if F.min_maf >= 0: keep &= c["maf"] >= F.min_maf
    if F.max_missing >= 0: keep &= c["miss"] <= F.max_missing
    if F.max_mendel_errors >= 0: keep &= c["merr"] <= F.max_mendel_errors
    if F.num_alleles >= 0: keep &= c["n_alleles"] == F.num_alleles
    if F.min_quality >= 0: keep &= c["qual"] >= F.min_quality
    return keep


def _run(host, vcf, ped, prefix, F, save, batch_bytes=1 << 22):
    host.hpgv_run_set_filters(C.byref(F))
    npass, nrej = C.c_long(-1), C.c_long(-1)
    try:
        rc = host.hpgv_run_filter(vcf.encode(), ped.encode() if ped else None, prefix.encode(), save, batch_bytes, C.byref(npass), C.byref(nrej))
    finally:
        host.hpgv_run_set_filters(None)
    assert rc == 0, host.hpgv_host_last_error()
    return open(prefix + ".filtered", "rb").read(), open(prefix + ".rejected", "rb").read(), npass.value, nrej.value


def _expected(c, F, keep, save):
    hdr = c["header"]
    cut = hdr.index(b"#CHROM")
    head = hdr[:cut] + _filter_lines(F) + hdr[cut:]
    kept = head + b"".join(l for l, k in zip(c["lines"], keep) if k)
    rej = head + b"".join(l for l, k in zip(c["lines"], keep) if not k) if save else b""
    return kept, rej


@pytest.mark.parametrize("which", list(FILTERS))
def test_each_filter_against_the_oracle(host, cohort, which):
    F = FILTERS[which]
    keep = _keep(cohort, F)
    assert 0 < keep.sum() < len(keep)
    for save in (0, 1):
        prefix = str(cohort["tmp"] / ("out_%s_%d" % (which, save)))
        got_f, got_r, npass, nrej = _run(host, cohort["paths"]["plain"], cohort["ped"], prefix, F, save)
        exp_f, exp_r = _expected(cohort, F, keep, save)
        assert got_f == exp_f
        assert got_r == exp_r
        assert npass == int(keep.sum()) and nrej == int((~keep).sum())


def test_plain_gzip_bgzip_and_small_batches_give_the_same_bytes(host, cohort):
    F = FILTERS["all"]
    keep = _keep(cohort, F)
    exp_f, exp_r = _expected(cohort, F, keep, 1)
    for kind in ("plain", "gzip", "bgzip"):
        for batch in (1 << 16, 1 << 22):
            prefix = str(cohort["tmp"] / ("same_%s_%d" % (kind, batch)))
            got_f, got_r, npass, nrej = _run(host, cohort["paths"][kind], cohort["ped"], prefix, F, 1, batch)
            assert got_f == exp_f, (kind, batch)
            assert got_r == exp_r, (kind, batch)
            assert npass == int(keep.sum()) and nrej == int((~keep).sum())
    t = (C.c_double * 6)()
    host.hpgv_host_last_run_times(t)
    assert t[5] >= 1 and t[4] > 0                              # batches and total time of the last run are reported


_CHILD = r"""
import ctypes as C, sys, importlib
sys.path.insert(0, %(root)r)
b = importlib.import_module("hpg-variant_amd._build")
L = C.CDLL(b.HOSTLIB)
class F(C.Structure):
    _fields_ = [("min_maf", C.c_double), ("max_missing", C.c_double), ("max_mendel_errors", C.c_int),
                ("num_alleles", C.c_int), ("min_quality", C.c_double)]
L.hpgv_run_filter.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
L.hpgv_run_set_filters.argtypes = [C.POINTER(F)]
L.hpgv_host_last_error.restype = C.c_char_p
vcf, ped, out = [a.encode() for a in sys.argv[1:4]]
f = F(0.02, 0.4, 50, 2, 5.0)
L.hpgv_run_set_filters(C.byref(f))
a, r = C.c_long(0), C.c_long(0)
rc = L.hpgv_run_filter(vcf, ped, out, 1, 1 << 16, C.byref(a), C.byref(r))
assert rc == 0, L.hpgv_host_last_error()
print(L.hpgv_host_device_count(), a.value, r.value)
L.hpgv_host_shutdown()
"""


def test_group_context_with_a_bgzip_file_staged_in_parts(cohort, tmp_path):
    F = FILTERS["all"]
    keep = _keep(cohort, F)
    exp_f, exp_r = _expected(cohort, F, keep, 1)
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"root": ROOT})
    env = {k: v for k, v in os.environ.items() if k != "HPGV_DEVICES"}
    env.update(HPGV_DEVICES="0,0", HPGV_RUN_TRACE="1", HPGV_BGZF_PART_MIN_KB="64")
    packed = cohort["paths"]["bgzip"]
    r = subprocess.run([sys.executable, str(script), packed, cohort["ped"], str(tmp_path / "grp")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    n_dev, npass, nrej = (int(x) for x in r.stdout.split())
    assert n_dev == 2 and npass == int(keep.sum()) and nrej == int((~keep).sum())
    if os.path.getsize(packed) >= 2 * (64 << 10):
        assert "stage: 2 parts, one per device" in r.stderr, r.stderr[-3000:]
    assert open(str(tmp_path / "grp") + ".filtered", "rb").read() == exp_f
    assert open(str(tmp_path / "grp") + ".rejected", "rb").read() == exp_r


@pytest.mark.parametrize("kind", ["plain", "bgzip"])
def test_last_line_without_newline_non_records_and_empty_lines(host, tmp_path, kind):
    rng = np.random.default_rng(4)
    hdr = b"##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\n"
    lines = []
    for v in range(3000):
        q = int(rng.integers(0, 60))
        lines.append(b"1\t%d\trs%d\tA\tC\t%d\tPASS\t.\tGT\t0/1\t1/1\n" % (100 + v, v, q))
    lines[10] = b"1\t110\n"                                      # not a record: rejected
    lines[20] = b"\n"                                           # empty: in neither file
    lines[21] = b"\n"
    lines[0] = b"\n"
    last = b"1\t999999\trs_last\tA\tC\t%d\tPASS\t.\tGT\t0/0\t0/1"   # no newline at the end of the file
    vcf = tmp_path / "in.vcf"
    F = _Filters(-1, -1, -1, -1, 30.0)
    for last_q in (45, 5):                                      # the unterminated line kept, then rejected
        data = hdr + b"".join(lines) + (last % last_q)
        vcf.write_bytes(data if kind == "plain" else _bgzf(data, 0x100))
        got_f, got_r, npass, nrej = _run(host, str(vcf), None, str(tmp_path / "o"), F, 1, 1 << 16)
        recs = [l for l in lines if l != b"\n"] + [(last % last_q) + b"\n"]
        ok = [l.count(b"\t") >= 5 and float(l.split(b"\t")[5]) >= 30.0 for l in recs]
        head = hdr[:hdr.index(b"#CHROM")] + _filter_lines(F) + hdr[hdr.index(b"#CHROM"):]
        assert got_f == head + b"".join(l for l, k in zip(recs, ok) if k)
        assert got_r == head + b"".join(l for l, k in zip(recs, ok) if not k)
        assert npass == sum(ok) and nrej == len(ok) - sum(ok)
