"""hpgv_run_split (hpg-var-vcf split, split_runner.c:23-190): every record to <out_dir>/<split name>_<base>, byte for byte,
against a small Python implementation of the rules of include/hpgv_host.h written here.  The directory listing and every
file's bytes are compared, from plain, gzip and bgzip input (the device decodes the bgzip file: more than 256 blocks), small
and large batches, a group context, more than 255 split names in one batch (the line ranges) and more than 64 over many
batches (files closed and reopened)."""
import ctypes as C
import gzip
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

from helpers import hpgv
from test_host_logic_cpu import _bgzf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHROMOSOME, COVERAGE = 1, 2
I64 = (-(1 << 63), (1 << 63) - 1)


@pytest.fixture(scope="module")
def host():
    hpgv.build()
    L = C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)
    L.hpgv_run_split.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_long), C.c_int, C.c_size_t,
                                 C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.hpgv_run_aggregate.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long)]
    L.hpgv_host_last_error.restype = C.c_char_p
    yield L
    L.hpgv_host_shutdown()


# ---- the rules, in Python ----
def _dp(info):
    for e in info.split(b";"):
        if e == b"DP":
            return None                                          # a bare flag
        if e.startswith(b"DP="):
            s, k, neg, m = e[3:], 0, False, 0
            if s[:1] in (b"+", b"-"):
                neg, k = s[:1] == b"-", 1
            while k < len(s) and 48 <= s[k] <= 57:
                m, k = m * 10 + s[k] - 48, k + 1
            return min(max(-m if neg else m, I64[0]), I64[1])
    return None


def _cov_name(v, iv):
    if v is None:
        return b"coverage_missing"
    if v <= iv[0]:
        return b"coverage_0_%d" % iv[0]
    for j in range(1, len(iv)):
        if v <= iv[j]:
            return b"coverage_%d_%d" % (iv[j - 1], iv[j])
    return b"coverage_%d_N" % iv[-1]


def expected(data, criterion, intervals, base):
    """{file name: bytes}, records, skipped lines"""
    cut = data.index(b"#CHROM")
    hdr = data[:data.index(b"\n", cut) + 1]
    body = data[len(hdr):]
    lines = body.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    files, skipped, records = {}, 0, 0
    for line in lines:
        f = line.split(b"\t")
        if len(f) < 8:
            skipped += 1
            continue
        name = b"chromosome_" + f[0] if criterion == CHROMOSOME else _cov_name(_dp(f[7]), intervals)
        files.setdefault(name.lower(), [name, []])[1].append(line + b"\n")
        records += 1
    out = {}
    for name, recs in files.values():
        fn = name.replace(b"%", b"%25").replace(b"/", b"%2F") + b"_" + base
        out[fn.decode("latin-1")] = hdr + b"".join(recs)
    return out, records, skipped


def run_split(host, vcf, out_dir, criterion, intervals=None, batch=1 << 22):
    iv = (C.c_long * max(1, len(intervals or [])))(*(intervals or []))
    nr, nf, ns = C.c_long(-1), C.c_long(-1), C.c_long(-1)
    rc = host.hpgv_run_split(str(vcf).encode(), str(out_dir).encode(), criterion, iv, len(intervals or []), batch,
                             C.byref(nr), C.byref(nf), C.byref(ns))
    assert rc == 0, host.hpgv_host_last_error()
    return nr.value, nf.value, ns.value


def check(host, data, vcf, out_dir, criterion, intervals=None, batch=1 << 22, base=None):
    base = base if base is not None else os.path.basename(str(vcf)).encode()
    for suffix in (b".gz", b".bgz"):
        if base.endswith(suffix):
            base = base[:-len(suffix)]
    exp, n_rec, n_skip = expected(data, criterion, intervals, base)
    nr, nf, ns = run_split(host, vcf, out_dir, criterion, intervals, batch)
    got = sorted(os.listdir(out_dir))
    assert got == sorted(exp), (sorted(set(got) ^ set(exp)))[:10]
    for fn, content in exp.items():
        with open(os.path.join(str(out_dir), fn), "rb") as f:
            assert f.read() == content, fn
    assert (nr, nf, ns) == (n_rec, len(exp), n_skip)
    return exp


INTERVALS = [-5, 0, 10, 20, 100]
DP_FORMS = [b"DP=%d", b"AC=1;DP=%d", b"DP=%d;AF=0.5", b"XDP=99;DP=%d", b"DPX=1;DP=%d;DP=1000"]
SPECIAL_INFO = [b".", b"DP", b"DP;DP=5", b"DP=", b"XDP=7", b"AC=3", b"DP=abc", b"DP=+7", b"DP=12abc", b"DP=-6", b"DP=-5",
                b"DP=99999999999999999999999", b"DP=-99999999999999999999", b"DP=0", b"DP=20", b"DP=100", b"DP=101",
                b"DP=10", b"DP=11", b"DP=-0", b"dp=3", b"DP=1;DP"]


def make_vcf(rng, n_rec, contigs, n_samples=20, order="runs", info=None):
    names = ["s%d" % j for j in range(n_samples)]
    hdr = ("##fileformat=VCFv4.1\n##source=test\n##contig=<ID=1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" +
           "\t".join(names) + "\n").encode()
    if order == "runs":
        chrom = [contigs[min(len(contigs) - 1, v * len(contigs) // n_rec)] for v in range(n_rec)]
    else:
        chrom = [contigs[int(k)] for k in rng.integers(0, len(contigs), n_rec)]
    lines = []
    for v in range(n_rec):
        if info is not None:
            inf = info(v)
        elif v % 3 == 0:
            inf = SPECIAL_INFO[v % len(SPECIAL_INFO)]
        else:
            inf = DP_FORMS[v % len(DP_FORMS)] % int(rng.integers(-10, 130))
        gts = b"\t".join([b"0/1", b"1/1", b"0/0", b"./."][int(k)] for k in rng.integers(0, 4, n_samples))
        lines.append(b"%s\t%d\trs%d\tA\tC\t50\tPASS\t%s\tGT\t%s\n" % (chrom[v], 100 + v, v, inf, gts))
    return hdr, lines


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """3 000 records of 20 samples (~250 KB; more than 256 bgzip blocks of 0x300 bytes) on 27 contigs in runs, chr1 / CHR1
    and Chr2 / chr2 among them, a CHROM with '/', one with '%'; the INFO forms of DP; empty lines, short lines, a line of
    exactly 8 fields, and a last line without a newline"""
    tmp = tmp_path_factory.mktemp("split")
    rng = np.random.default_rng(17)
    contigs = [b"chr%d" % k for k in range(1, 23)] + [b"chrX", b"CHR1", b"chrUn/gl000220", b"odd%name", b"chr2"]
    contigs[1] = b"Chr2"
    hdr, lines = make_vcf(rng, 3000, contigs)
    lines[10] = b"\n"
    lines[11] = b"chr1\t100\n"
    lines[500] = b"chr3\t5\trs\tA\tC\t9\tPASS\n"                       # 7 fields: no file
    lines[501] = b"chr3\t5\trsx\tA\tC\t9\tPASS\tDP=15\n"               # 8 fields: a record
    lines[1500] = b"\n"
    lines[2999] = lines[2999].rstrip(b"\n")                            # no newline at the end of the file
    data = hdr + b"".join(lines)
    paths = {"plain": tmp / "in.vcf", "gzip": tmp / "gz_in.vcf.gz", "bgzip": tmp / "bg_in.vcf.bgz"}
    paths["plain"].write_bytes(data)
    paths["gzip"].write_bytes(gzip.compress(data, 6))
    paths["bgzip"].write_bytes(_bgzf(data, 0x300))
    assert len(data) // 0x300 > 256
    return dict(tmp=tmp, data=data, paths=paths)


@pytest.mark.parametrize("criterion", [CHROMOSOME, COVERAGE])
@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzip"])
@pytest.mark.parametrize("batch", [1 << 16, 1 << 22])
def test_plain_gzip_bgzip_and_batches(host, files, tmp_path, criterion, kind, batch):
    exp = check(host, files["data"], files["paths"][kind], tmp_path / "out", criterion,
                INTERVALS if criterion == COVERAGE else None, batch)
    if criterion == CHROMOSOME:
        base = {"plain": "in.vcf", "gzip": "gz_in.vcf", "bgzip": "bg_in.vcf"}[kind]
        assert "chromosome_chr1_" + base in exp and "chromosome_CHR1_" + base not in exp      # named after the first
        assert "chromosome_Chr2_" + base in exp and "chromosome_chr2_" + base not in exp
        assert "chromosome_chrUn%2Fgl000220_" + base in exp and "chromosome_odd%25name_" + base in exp
    else:
        assert len(exp) == len(INTERVALS) + 2


def test_interval_bounds_one_record_each(host, tmp_path):
    vals = [-7, -6, -5, -4, -1, 0, 1, 9, 10, 11, 19, 20, 21, 99, 100, 101, 10 ** 6]
    hdr, lines = make_vcf(np.random.default_rng(1), len(vals), [b"1"], 2, info=lambda v: b"DP=%d" % vals[v])
    vcf = tmp_path / "b.vcf"
    vcf.write_bytes(hdr + b"".join(lines))
    exp = check(host, hdr + b"".join(lines), vcf, tmp_path / "o", COVERAGE, INTERVALS)
    assert sorted(exp) == sorted("%s_b.vcf" % n for n in ("coverage_0_-5", "coverage_-5_0", "coverage_0_10", "coverage_10_20",
                                                           "coverage_20_100", "coverage_100_N"))
    check(host, hdr + b"".join(lines), vcf, tmp_path / "one", COVERAGE, [15])


def test_more_than_255_contigs_in_one_batch(host, tmp_path):
    rng = np.random.default_rng(2)
    contigs = [b"ctg%d" % k for k in range(700)] + [b"CTG%d" % k for k in range(0, 700, 7)]
    hdr, lines = make_vcf(rng, 6000, contigs, 4, order="random")
    data = hdr + b"".join(lines)
    vcf = tmp_path / "many.vcf"
    vcf.write_bytes(data)
    check(host, data, vcf, tmp_path / "o", CHROMOSOME)              # one batch: three line ranges at least
    check(host, data, vcf, tmp_path / "small", CHROMOSOME, batch=1 << 16)


def test_more_than_64_contigs_over_batches_reopen(host, tmp_path):
    rng = np.random.default_rng(3)
    contigs = [b"scaffold_%d" % k for k in range(150)]
    hdr, lines = make_vcf(rng, 5000, contigs, 30, order="random")
    runs = [l.replace(b"scaffold_", b"run_") for l in make_vcf(rng, 3000, contigs, 30)[1]]
    data = hdr + b"".join(lines + runs)
    vcf = tmp_path / "reopen.vcf.gz"
    vcf.write_bytes(_bgzf(data, 0x400))
    check(host, data, vcf, tmp_path / "o", CHROMOSOME, batch=1 << 16)


def test_sites_only_input_from_aggregate(host, files, tmp_path):
    agg = tmp_path / "agg.vcf"
    n = C.c_long(0)
    assert host.hpgv_run_aggregate(str(files["paths"]["plain"]).encode(), str(agg).encode(), 0, 1 << 20, C.byref(n)) == 0, \
        host.hpgv_host_last_error()
    data = agg.read_bytes()
    assert data.split(b"\n")[-2].count(b"\t") == 7                    # 8 columns, no samples
    check(host, data, agg, tmp_path / "chr", CHROMOSOME)
    check(host, data, agg, tmp_path / "cov", COVERAGE, INTERVALS, batch=1 << 16)


def test_existing_out_dir_and_rerun_truncates(host, files, tmp_path):
    out = tmp_path / "o"
    out.mkdir()
    check(host, files["data"], files["paths"]["plain"], out, COVERAGE, INTERVALS)
    check(host, files["data"], files["paths"]["plain"], out, COVERAGE, INTERVALS, batch=1 << 16)   # same files, not appended to


_CHILD = r"""
import ctypes as C, sys, importlib
sys.path.insert(0, %(root)r)
b = importlib.import_module("hpg-variant_amd._build")
L = C.CDLL(b.HOSTLIB)
L.hpgv_run_split.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_long), C.c_int, C.c_size_t,
                             C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]
L.hpgv_host_last_error.restype = C.c_char_p
vcf, out, crit = sys.argv[1].encode(), sys.argv[2].encode(), int(sys.argv[3])
iv = (C.c_long * 5)(-5, 0, 10, 20, 100)
a, f, s = C.c_long(0), C.c_long(0), C.c_long(0)
rc = L.hpgv_run_split(vcf, out, crit, iv, 5, 1 << 16, C.byref(a), C.byref(f), C.byref(s))
assert rc == 0, L.hpgv_host_last_error()
print(L.hpgv_host_device_count(), a.value, f.value, s.value)
L.hpgv_host_shutdown()
"""


@pytest.mark.parametrize("criterion", [CHROMOSOME, COVERAGE])
def test_group_context_with_a_bgzip_file_staged_in_parts(files, tmp_path, criterion):
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"root": ROOT})
    env = {k: v for k, v in os.environ.items() if k != "HPGV_DEVICES"}
    env.update(HPGV_DEVICES="0,0", HPGV_RUN_TRACE="1", HPGV_BGZF_PART_MIN_KB="64")
    packed = str(files["paths"]["bgzip"])
    out = tmp_path / "grp"
    r = subprocess.run([sys.executable, str(script), packed, str(out), str(criterion)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    n_dev, nr, nf, ns = (int(x) for x in r.stdout.split())
    exp, n_rec, n_skip = expected(files["data"], criterion, INTERVALS, b"bg_in.vcf")
    assert n_dev == 2 and (nr, nf, ns) == (n_rec, len(exp), n_skip)
    if os.path.getsize(packed) >= 2 * (64 << 10):
        assert "stage: 2 parts, one per device" in r.stderr, r.stderr[-3000:]
    assert sorted(os.listdir(out)) == sorted(exp)
    for fn, content in exp.items():
        assert (out / fn).read_bytes() == content, fn
