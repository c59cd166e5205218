"""The record filters of hpgv_run_set_record_filters in the file runners: hpgv_run_filter's .filtered / .rejected byte for
byte against a Python model of the definitions (include/hpgv_host.h, include/hpgv.h), each new filter alone, all together,
and all together with the old ones, from plain, gzip and bgzip input in small batches and from a group context; then
assoc, tdt and vcf2epi with filters, and stats and split unchanged by them."""
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
from test_inheritance_scan_gpu import model as inherit_counts
from test_record_filters_cpu import _RecFilters, rec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Filters(C.Structure):
    _fields_ = [("min_maf", C.c_double), ("max_missing", C.c_double), ("max_mendel_errors", C.c_int),
                ("num_alleles", C.c_int), ("min_quality", C.c_double)]


OFF = _Filters(-1, -1, -1, -1, -1)
REGIONS = "1:1010-1400,2,chr3:1600,1:1300-1500,1:1700-1700"
GFF = ("##gff-version 3\n#comment\n\n"
       "1\tsrc\tgene\t1100\t1199\t.\t+\t.\tID=g1\n"
       "1\tsrc\texon\t1150\t1250\t.\t+\t.\tID=e1\n"
       "2\tsrc\tgene\t1000\t1400\t.\t-\t.\tID=g2\n"
       "chr3\tsrc\texon\t1000\t2199\t.\t+\t.\tID=e2\n"
       "2\tsrc\texon\t1401\t1401\t.\t+\t.\tID=e3\n")
# REF, ALT: SNVs, multi-allelic SNVs, indels, an MNP, symbolic and breakend alleles, a spanning '*', no ALT
ALLELES = [("A", "C"), ("A", "C,G"), ("A", "AT"), ("AT", "A"), ("AT", "GC"), ("A", "<DEL>"), ("G", "G]17:198982]"), ("A", "."),
           ("C", "C,<NON_REF>"), ("A", "[13:123457[A"), ("AC", "A,AGT"), ("T", "*"), ("AG", "TC,T")]
INFOS = ["DP=%d", "AC=1;DP=%d", "DP", ".", "NS=3;DP=%d;AF=0.5", "DPX=%d", "AF=0.1"]


def _keep_fields(c, F):
    """the model of the field filters of hpgv_run_set_record_filters"""
    out = []
    for r in c["recs"]:
        ok = True
        if F.get("regions"):
            ok &= _in_regions(_parse_regions(F["regions"]), r["chrom"], r["pos"])
        if F.get("region_file"):
            ok &= _in_regions(_parse_gff(c["gff"], F.get("region_type")), r["chrom"], r["pos"])
        if F.get("min_coverage", -1) >= 0:
            ok &= r["dp"] is not None and r["dp"] >= F["min_coverage"]
        if F.get("snp", -1) >= 0:
            ok &= (r["id"] != ".") == (F["snp"] == 1)
        t = _var_type(r["ref"], r["alt"])
        if F.get("var_type", -1) >= 0:
            ok &= t == F["var_type"]
        if F.get("indel", -1) >= 0:
            ok &= (t == 2) == (F["indel"] == 1)
        out.append(ok)
    return np.array(out, bool)


def _parse_regions(s):
    out = []
    for item in s.split(","):
        if ":" in item:
            ch, rng = item.rsplit(":", 1)
            lo, hi = (int(x) for x in rng.split("-")) if "-" in rng else (int(rng), int(rng))
        else:
            ch, lo, hi = item, -(1 << 62), 1 << 62
        out.append((ch, lo, hi))
    return out


def _parse_gff(text, typ):
    out = []
    for line in text.splitlines():
        if not line or line.startswith("#"):
            continue
        f = line.split("\t")
        if typ is None or f[2] == typ:
            out.append((f[0], int(f[3]), int(f[4])))
    return out


def _in_regions(regs, chrom, pos):
    return any(ch == chrom and lo <= pos <= hi for ch, lo, hi in regs)


def _var_type(ref, alt):
    if alt == "." or not alt:
        return 0
    al = alt.split(",")
    if any(a.startswith("<") or "[" in a or "]" in a for a in al):
        return 3
    if len(ref) == 1 and all(len(a) == 1 and a != "." for a in al):
        return 1
    return 2 if any(len(a) != len(ref) for a in al) else 0


def _keep_inherit(c, dom, rec_, epi=False):
    cond = c["cond"]
    if epi:
        cond = np.where(cond == hpgv.COND_AFFECTED, hpgv.COND_AFFECTED, hpgv.COND_UNAFFECTED).astype(np.uint8)
    k = inherit_counts(c["strict"], cond).astype(np.int64)
    den = k[:, 0] + k[:, 3]
    keep = den > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        if dom >= 0:
            keep &= (k[:, 1] + k[:, 4]) / den >= dom
        if rec_ >= 0:
            keep &= (k[:, 2] + (k[:, 3] - k[:, 5])) / den >= rec_
    return keep


def _keep_old(c, F):
    keep = np.ones(len(c["lines"]), bool)
    if F.min_maf >= 0: keep &= c["maf"] >= F.min_maf
    if F.max_missing >= 0: keep &= c["miss"] <= F.max_missing
    if F.max_mendel_errors >= 0: keep &= c["merr"] <= F.max_mendel_errors
    if F.num_alleles >= 0: keep &= c["n_alleles"] == F.num_alleles
    if F.min_quality >= 0: keep &= c["qual"] >= F.min_quality
    return keep


def keep_of(c, R, F=OFF, epi=False):
    k = _keep_fields(c, R) & _keep_old(c, F)
    if R.get("min_dominant", -1) >= 0 or R.get("min_recessive", -1) >= 0:
        k &= _keep_inherit(c, R.get("min_dominant", -1), R.get("min_recessive", -1), epi)
    return k


def _esc(s):
    return s.replace("\\", "\\\\").replace('"', '\\"')


def filter_lines(F, R):
    out = []
    if F.min_maf >= 0: out.append('##FILTER=<ID=maf,Description="Minor allele frequency >= %g">\n' % F.min_maf)
    if F.max_missing >= 0: out.append('##FILTER=<ID=missing,Description="Rate of missing genotypes <= %g">\n' % F.max_missing)
    if F.max_mendel_errors >= 0: out.append('##FILTER=<ID=mendel,Description="Mendelian errors <= %g">\n' % F.max_mendel_errors)
    if F.num_alleles >= 0: out.append('##FILTER=<ID=alleles,Description="Number of alleles == %g">\n' % F.num_alleles)
    if F.min_quality >= 0: out.append('##FILTER=<ID=quality,Description="Quality >= %g">\n' % F.min_quality)
    if R.get("min_coverage", -1) >= 0: out.append('##FILTER=<ID=coverage,Description="Coverage >= %d">\n' % R["min_coverage"])
    if R.get("regions"): out.append('##FILTER=<ID=region,Description="Regions %s">\n' % _esc(R["regions"]))
    if R.get("region_file"):
        t = R.get("region_type")
        out.append('##FILTER=<ID=region-file,Description="Regions of file %s%s">\n' % (_esc(R["region_file"]), " of type " + _esc(t) if t else ""))
    if R.get("snp", -1) >= 0: out.append('##FILTER=<ID=snp,Description="SNP %s">\n' % ("include" if R["snp"] else "exclude"))
    if R.get("var_type", -1) >= 0: out.append('##FILTER=<ID=var-type,Description="Variant type == %s">\n' % ["", "snv", "indel", "structural"][R["var_type"]])
    if R.get("indel", -1) >= 0: out.append('##FILTER=<ID=indel,Description="Indels %s">\n' % ("include" if R["indel"] else "exclude"))
    if R.get("min_dominant", -1) >= 0:
        out.append('##FILTER=<ID=inh-dom,Description="Samples following a dominant inheritance pattern >= %g">\n' % R["min_dominant"])
    if R.get("min_recessive", -1) >= 0:
        out.append('##FILTER=<ID=inh-rec,Description="Samples following a recessive inheritance pattern >= %g">\n' % R["min_recessive"])
    return "".join(out).encode()


@pytest.fixture(scope="module")
def host():
    hpgv.build()
    L = C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)
    L.hpgv_run_filter.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.hpgv_run_assoc.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long)]
    L.hpgv_run_tdt.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_long)]
    L.hpgv_run_vcf2epi.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_long)]
    L.hpgv_run_stats.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_long)]
    L.hpgv_run_split.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_long), C.c_int, C.c_size_t,
                                 C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.hpgv_run_set_filters.argtypes = [C.POINTER(_Filters)]
    L.hpgv_run_set_record_filters.argtypes = [C.POINTER(_RecFilters)]
    L.hpgv_host_last_error.restype = C.c_char_p
    yield L
    L.hpgv_run_set_filters(None)
    L.hpgv_run_set_record_filters(None)
    L.hpgv_host_shutdown()


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    """1 500 records of ~110 samples over chromosomes 1, 2 and chr3 at positions on and around the region bounds, with every
    kind of ALT allele, records without DP, '.' IDs; the old filters' oracle values too"""
    tmp = tmp_path_factory.mktemp("recfilt")
    rng = np.random.default_rng(77)
    people, names, rows = _write_inputs(tmp, rng, 22, 20, 1500, chroms=("1", "2", "chr3"))
    n = len(names)
    recs, lines = [], []
    for v, (chrom, fmt, samples) in enumerate(rows):
        gpos = fmt.split(":").index("GT")
        if v % 6 == 0:                                           # carriers among the affected more often: inheritance fractions spread
            for k in range(n):
                if rng.random() < 0.5:
                    parts = samples[k].split(":"); parts[gpos] = ["0/1", "1/1", "0/0"][v // 6 % 3]; samples[k] = ":".join(parts)
        pos = 1000 + v // 3 * 2                                  # 1000 .. 1998 per chromosome, hitting every bound above
        ref, alt = ALLELES[int(rng.integers(0, len(ALLELES)))]
        dpv = int(rng.integers(0, 40))
        info = INFOS[v % len(INFOS)]
        info = info % dpv if "%d" in info else info
        dp = dpv if info.startswith("DP=") or ";DP=" in info else None
        rid = "." if v % 4 == 0 else "rs%d" % v
        qual = [".", "10", "35.5", "90"][v % 4 if v % 5 else 3]
        recs.append(dict(chrom=chrom, pos=pos, id=rid, ref=ref, alt=alt, dp=dp))
        lines.append(("%s\t%d\t%s\t%s\t%s\t%s\tPASS\t%s\t%s\t%s\n" % (chrom, pos, rid, ref, alt, qual, info, fmt, "\t".join(samples))).encode())
    header = ("##fileformat=VCFv4.1\n##source=test\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n").encode()
    lax = np.array([[orc.encode_sample(s, fmt.split(":").index("GT"), False) for s in samples] for _, fmt, samples in rows], np.uint8)
    strict = np.where(((lax >> 4) == 0xF) | ((lax & 0xF) == 0xF), 0xFF, lax).astype(np.uint8)
    pheno = {p[1]: p[5] for p in people}
    cond = np.array([hpgv.COND_AFFECTED if pheno[nm] == 2 else hpgv.COND_UNAFFECTED if pheno[nm] == 1 else hpgv.COND_OTHER
                     for nm in names], np.uint8)
    is_x = np.zeros(len(rows), np.uint8)
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
    n_alleles = np.array([1 if r["alt"] == "." else 1 + len(r["alt"].split(",")) for r in recs])
    qual = np.array([-1.0 if l.split(b"\t")[5] == b"." else float(l.split(b"\t")[5]) for l in lines])
    data = header + b"".join(lines)
    paths = {"plain": tmp / "in.vcf", "gzip": tmp / "in.vcf.gzip.gz", "bgzip": tmp / "in.vcf.gz"}
    paths["plain"].write_bytes(data)
    paths["gzip"].write_bytes(gzip.compress(data, 6))
    paths["bgzip"].write_bytes(_bgzf(data, 0x700))
    (tmp / "regions.gff").write_text(GFF)
    return dict(tmp=tmp, header=header, lines=lines, recs=recs, ped=str(tmp / "ped.txt"), paths={k: str(v) for k, v in paths.items()},
                gff=GFF, gff_path=str(tmp / "regions.gff"), cond=cond, strict=strict, merr=merr, maf=maf, miss=miss,
                n_alleles=n_alleles, qual=qual)


def _set(host, c, R, F=OFF):
    R = dict(R)
    if R.get("region_file") == "GFF":
        R["region_file"] = c["gff_path"]
    assert host.hpgv_run_set_record_filters(C.byref(rec(**R))) == 0, host.hpgv_host_last_error()
    host.hpgv_run_set_filters(C.byref(F))
    return R


def _run_filter(host, c, vcf, prefix, R, F=OFF, batch=1 << 22, save=1):
    R = _set(host, c, R, F)
    npass, nrej = C.c_long(-1), C.c_long(-1)
    try:
        rc = host.hpgv_run_filter(vcf.encode(), c["ped"].encode(), prefix.encode(), save, batch, C.byref(npass), C.byref(nrej))
    finally:
        host.hpgv_run_set_filters(None); host.hpgv_run_set_record_filters(None)
    assert rc == 0, host.hpgv_host_last_error()
    return R, open(prefix + ".filtered", "rb").read(), open(prefix + ".rejected", "rb").read(), npass.value, nrej.value


def _expected(c, R, F, keep):
    hdr = c["header"]
    cut = hdr.index(b"#CHROM")
    head = hdr[:cut] + filter_lines(F, R) + hdr[cut:]
    return (head + b"".join(l for l, k in zip(c["lines"], keep) if k),
            head + b"".join(l for l, k in zip(c["lines"], keep) if not k))


ALONE = {
    "coverage": dict(min_coverage=12), "coverage0": dict(min_coverage=0), "region": dict(regions=REGIONS),
    "region_file": dict(region_file="GFF"), "region_type": dict(region_file="GFF", region_type="exon"),
    "snp_in": dict(snp=1), "snp_ex": dict(snp=0), "snv": dict(var_type=1), "indel_type": dict(var_type=2),
    "structural": dict(var_type=3), "indel_in": dict(indel=1), "indel_ex": dict(indel=0),
    "inh_dom": dict(min_dominant=0.6), "inh_rec": dict(min_recessive=0.5),
    "region_and_file": dict(regions=REGIONS, region_file="GFF"),
}
ALL_NEW = dict(min_coverage=3, regions="1,2:1000-1900,chr3", region_file="GFF", region_type="gene", snp=1, indel=0,
               min_dominant=0.3, min_recessive=0.2)
ALL_OLD = _Filters(0.02, 0.4, 50, -1, 36.0)


@pytest.mark.parametrize("which", list(ALONE))
def test_each_new_filter_alone(host, cohort, which):
    R0 = ALONE[which]
    prefix = str(cohort["tmp"] / ("alone_" + which))
    R, got_f, got_r, npass, nrej = _run_filter(host, cohort, cohort["paths"]["plain"], prefix, R0)
    keep = keep_of(cohort, R)
    assert 0 < keep.sum() < len(keep), which
    exp_f, exp_r = _expected(cohort, R, OFF, keep)
    assert got_f == exp_f
    assert got_r == exp_r
    assert npass == int(keep.sum()) and nrej == int((~keep).sum())


@pytest.mark.parametrize("with_old", [False, True])
def test_all_together_every_input_small_batches(host, cohort, with_old):
    F = ALL_OLD if with_old else OFF
    exp = None
    for kind in ("plain", "gzip", "bgzip"):
        for batch in (1 << 16, 1 << 22):
            prefix = str(cohort["tmp"] / ("all_%d_%s_%d" % (with_old, kind, batch)))
            R, got_f, got_r, npass, nrej = _run_filter(host, cohort, cohort["paths"][kind], prefix, ALL_NEW, F, batch)
            if exp is None:
                keep = keep_of(cohort, R, F)
                assert keep.sum() > 0
                exp = _expected(cohort, R, F, keep)
            assert got_f == exp[0], (kind, batch)
            assert got_r == exp[1], (kind, batch)
            assert npass == int(keep.sum()) and nrej == int((~keep).sum())


def test_filter_lines_escape_quotes_and_backslashes(host, cohort, tmp_path):
    gff = tmp_path / 'odd "name"\\x.gff'
    gff.write_text(GFF)
    R = dict(regions="1:1000-1100", region_file=str(gff), region_type="exon", var_type=3, snp=0, indel=1)
    R, got_f, _, _, _ = _run_filter(host, cohort, cohort["paths"]["plain"], str(tmp_path / "esc"), R)
    assert b'##FILTER=<ID=region-file,Description="Regions of file ' + _esc(str(gff)).encode() + b' of type exon">\n' in got_f
    exp_f, _ = _expected(cohort, R, OFF, keep_of(cohort, R))
    assert got_f == exp_f


_CHILD = r"""
import ctypes as C, sys, importlib
sys.path.insert(0, %(root)r)
class RF(C.Structure):
    _fields_ = [("min_coverage", C.c_long), ("regions", C.c_char_p), ("region_file", C.c_char_p), ("region_type", C.c_char_p),
                ("snp", C.c_int), ("var_type", C.c_int), ("indel", C.c_int), ("min_dominant", C.c_double), ("min_recessive", C.c_double)]
b = importlib.import_module("hpg-variant_amd._build")
L = C.CDLL(b.HOSTLIB)
class F(C.Structure):
    _fields_ = [("min_maf", C.c_double), ("max_missing", C.c_double), ("max_mendel_errors", C.c_int),
                ("num_alleles", C.c_int), ("min_quality", C.c_double)]
L.hpgv_run_filter.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
L.hpgv_run_set_filters.argtypes = [C.POINTER(F)]
L.hpgv_run_set_record_filters.argtypes = [C.POINTER(RF)]
L.hpgv_host_last_error.restype = C.c_char_p
vcf, ped, out, gff = [a.encode() for a in sys.argv[1:5]]
f = F(0.02, 0.4, 50, -1, 36.0)
L.hpgv_run_set_filters(C.byref(f))
r = RF(3, b"1,2:1000-1900,chr3", gff, b"gene", 1, -1, 0, 0.3, 0.2)
assert L.hpgv_run_set_record_filters(C.byref(r)) == 0
a, j = C.c_long(0), C.c_long(0)
rc = L.hpgv_run_filter(vcf, ped, out, 1, 1 << 16, C.byref(a), C.byref(j))
assert rc == 0, L.hpgv_host_last_error()
print(L.hpgv_host_device_count(), a.value, j.value)
L.hpgv_host_shutdown()
"""


def test_group_context(cohort, tmp_path):
    R = dict(ALL_NEW, region_file=cohort["gff_path"])
    keep = keep_of(cohort, R, ALL_OLD)
    exp_f, exp_r = _expected(cohort, R, ALL_OLD, keep)
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"root": ROOT})
    env = {k: v for k, v in os.environ.items() if k != "HPGV_DEVICES"}
    env.update(HPGV_DEVICES="0,0", HPGV_BGZF_PART_MIN_KB="64")
    r = subprocess.run([sys.executable, str(script), cohort["paths"]["bgzip"], cohort["ped"], str(tmp_path / "grp"), cohort["gff_path"]],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    n_dev, npass, nrej = (int(x) for x in r.stdout.split())
    assert n_dev == 2 and npass == int(keep.sum()) and nrej == int((~keep).sum())
    assert open(str(tmp_path / "grp") + ".filtered", "rb").read() == exp_f
    assert open(str(tmp_path / "grp") + ".rejected", "rb").read() == exp_r


def _key(line):
    f = line.split(b"\t")
    return f[0], int(f[1])


def test_assoc_with_region_and_inheritance_is_the_unfiltered_run_restricted(host, cohort, tmp_path):
    c = cohort
    n = C.c_long(-1)
    host.hpgv_run_set_record_filters(None)
    assert host.hpgv_run_assoc(c["paths"]["plain"].encode(), c["ped"].encode(), str(tmp_path / "all.assoc").encode(), 1, 1 << 16, C.byref(n)) == 0
    R = _set(host, c, dict(regions=REGIONS, min_dominant=0.5))
    host.hpgv_run_set_filters(None)
    try:
        rc = host.hpgv_run_assoc(c["paths"]["bgzip"].encode(), c["ped"].encode(), str(tmp_path / "some.assoc").encode(), 1, 1 << 16, C.byref(n))
    finally:
        host.hpgv_run_set_record_filters(None)
    assert rc == 0, host.hpgv_host_last_error()
    keep = keep_of(c, R)
    assert 0 < keep.sum() < len(keep) and n.value == int(keep.sum())
    kept = {(r["chrom"].encode(), r["pos"]) for r, k in zip(c["recs"], keep) if k}
    full = open(tmp_path / "all.assoc", "rb").read().splitlines(keepends=True)
    body = [l for l in full if not l.startswith(b"#")]
    exp = [l for l in full if l.startswith(b"#")] + [l for l in body if _key(l) in kept]
    assert open(tmp_path / "some.assoc", "rb").read() == b"".join(exp)


def test_tdt_and_vcf2epi_report_the_kept_count(host, cohort, tmp_path):
    c = cohort
    R = _set(host, c, dict(regions="1:1000-1500,chr3", min_dominant=0.45, min_recessive=0.1, snp=1))
    host.hpgv_run_set_filters(None)
    n_tdt, n_epi = C.c_long(-1), C.c_long(-1)
    try:
        rc1 = host.hpgv_run_tdt(c["paths"]["gzip"].encode(), c["ped"].encode(), str(tmp_path / "t.tdt").encode(), 1 << 16, C.byref(n_tdt))
        rc2 = host.hpgv_run_vcf2epi(c["paths"]["plain"].encode(), c["ped"].encode(), str(tmp_path / "e.bin").encode(), 1 << 16, C.byref(n_epi))
    finally:
        host.hpgv_run_set_record_filters(None)
    assert rc1 == 0 and rc2 == 0, host.hpgv_host_last_error()
    k_tdt, k_epi = keep_of(c, R), keep_of(c, R, epi=True)
    assert 0 < k_tdt.sum() < len(k_tdt)
    assert n_tdt.value == int(k_tdt.sum())
    assert n_epi.value == int(k_epi.sum())
    data = open(tmp_path / "e.bin", "rb").read()
    nv, na, nu = np.frombuffer(data[:12], np.uint32)
    assert nv == int(k_epi.sum()) and len(data) == 12 + nv * (na + nu)
    tdt_lines = [l for l in open(tmp_path / "t.tdt", "rb").read().splitlines() if not l.startswith(b"#")]
    assert len(tdt_lines) == int(k_tdt.sum())


def _tree(d):
    return {os.path.relpath(os.path.join(r, f), d): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(d) for f in fs}


def test_stats_and_split_ignore_the_new_filters(host, cohort, tmp_path):
    c = cohort
    outs = []
    for on in (False, True):
        d = tmp_path / ("on" if on else "off")
        d.mkdir()
        if on:
            _set(host, c, dict(ALL_NEW, region_file="GFF"))
            host.hpgv_run_set_filters(None)
        n = C.c_long(-1)
        try:
            assert host.hpgv_run_stats(c["paths"]["plain"].encode(), c["ped"].encode(), str(d / "st").encode(), 1 << 16, C.byref(n)) == 0
            iv = (C.c_long * 2)(10, 20)
            nr, nf, ns = C.c_long(), C.c_long(), C.c_long()
            assert host.hpgv_run_split(c["paths"]["plain"].encode(), str(d / "split").encode(), 2, iv, 2, 1 << 16,
                                       C.byref(nr), C.byref(nf), C.byref(ns)) == 0
        finally:
            host.hpgv_run_set_record_filters(None)
        outs.append((_tree(d), n.value, nr.value))
    assert outs[0] == outs[1]
    assert outs[0][1] == len(c["lines"]) and outs[0][2] == len(c["lines"])
