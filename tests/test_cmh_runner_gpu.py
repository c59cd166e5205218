"""hpgv_run_assoc_cmh: the stratified association's file runner.  Its file is cmh_golden's oracle of every record, formatted line by
line -- rows on chromosome X by their rule -- whatever the batch size and the input form; a sample missing from the within file
leaves the cohort; with one stratum for everyone the autosomal CHISQ_CMH is (n - 1) / n x the .chisq file's CHISQ."""
import ctypes as C
import gzip
import os
import subprocess
from importlib import import_module

import numpy as np
import pytest

import cmh_golden as cg
from helpers import hpgv

pytestmark = pytest.mark.gpu

HEADER = "#CHR\tPOS\tID\tA1\tA2\tNSTRATA\tCHISQ_CMH\tP_CMH\tOR_MH\tSE\tL95\tU95\tCHISQ_BD\tP_BD\n"
N_SAMPLES, N_RECORDS = 40, 60
CODE = {"0/0": 0x00, "0/1": 0x01, "1/0": 0x10, "1/1": 0x11, "./.": 0xFF}
CLUSTERS = ["north", "south", "east"]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cmh_runner")
    rng = np.random.default_rng(91)
    names = ["S%d" % i for i in rng.permutation(N_SAMPLES)]
    pheno = rng.choice([1, 2, 2, 1, 0], N_SAMPLES)                   # 0: in no class
    with open(tmp / "ped.txt", "w") as f:
        for k in rng.permutation(N_SAMPLES):                         # PED order is not the VCF's
            f.write("fam%d %s 0 0 %d %d\n" % (k, names[k], 1 + k % 2, pheno[k]))
    cluster = rng.integers(0, 3, N_SAMPLES)
    cohort = np.flatnonzero(pheno != 0)
    absent = int(cohort[4])                                          # one cohort sample without a line
    with open(tmp / "within.txt", "w") as f:
        f.write("FID IID CLUSTER\n")
        for k in rng.permutation(N_SAMPLES):
            if k != absent:
                f.write("fam%d\t%s  %s\n" % (k, names[k], CLUSTERS[cluster[k]]))
        f.write("famX nobody west\n")                                # a line of a sample the VCF does not have
    with open(tmp / "one.txt", "w") as f:                            # one stratum for everyone
        for k in range(N_SAMPLES):
            f.write("fam%d %s all\n" % (k, names[k]))
    gts = np.array(list(CODE))
    rows, lines = [], []
    for v in range(N_RECORDS):
        chrom = ("1", "X", "22", "3")[v % 4]
        g = gts[rng.choice(5, N_SAMPLES, p=[0.3, 0.2, 0.2, 0.25, 0.05])]
        if v == 7:
            g[:] = "0/0"                                              # monomorphic: nan in the file
        rows.append((chrom, 5000 - 13 * v, "rs%d" % v, np.array([CODE[x] for x in g], np.uint8)))      # positions fall: the file is sorted afterwards
        lines.append("%s\t%d\trs%d\tA\tC\t.\tPASS\t.\tGT\t%s\n" % (chrom, 5000 - 13 * v, v, "\t".join(g)))
    head = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n"
    data = (head + "".join(lines)).encode()
    paths = dict(plain=str(tmp / "in.vcf"), gzip=str(tmp / "in_gz.vcf.gz"))
    open(paths["plain"], "wb").write(data)
    open(paths["gzip"], "wb").write(gzip.compress(data))
    return dict(tmp=tmp, paths=paths, ped=str(tmp / "ped.txt"), within=str(tmp / "within.txt"), one=str(tmp / "one.txt"), names=names, pheno=pheno,
                cluster=cluster, rows=rows, absent=absent)


def _sorted(text):
    return subprocess.run(["sort", "-k1,1h", "-k2,2n"], input=text.encode(), capture_output=True, env=dict(os.environ, LC_ALL="C"), check=True).stdout


def _records(inputs, stratum, K):
    """the oracle's record of every row for the strata given per VCF column (-1: not in the cohort)"""
    cond = np.where(stratum < 0, 2, np.where(inputs["pheno"] == 2, 1, 0)).astype(np.uint8)
    codes = np.stack([r[3] for r in inputs["rows"]])
    is_x = np.array([r[0] == "X" for r in inputs["rows"]], np.uint8)
    return [cg.fit(t) for t in cg.tables(codes, cond, stratum, K, is_x)]


def _strata(inputs):
    """the runner's numbering: by first appearance in VCF column order among the cohort samples with a line"""
    stratum, seen = np.full(N_SAMPLES, -1, np.int32), {}
    for j in range(N_SAMPLES):
        if inputs["pheno"][j] != 0 and j != inputs["absent"]:
            stratum[j] = seen.setdefault(int(inputs["cluster"][j]), len(seen))
    return stratum, len(seen)


@pytest.fixture(scope="module")
def expected(inputs):
    stratum, K = _strata(inputs)
    recs = _records(inputs, stratum, K)
    assert K == 3 and sum(r["chisq_bd"] == r["chisq_bd"] for r in recs) >= N_RECORDS // 2      # the comparison says something
    text = HEADER + "".join(cg.format_line(chrom, pos, vid, "A", "C", r) + "\n" for (chrom, pos, vid, _), r in zip(inputs["rows"], recs))
    return _sorted(text), int((stratum >= 0).sum()), K


def test_the_file_is_the_oracles_whatever_the_batch_and_the_form(inputs, expected):
    files = []
    for form, batch in [("plain", 1 << 16), ("plain", 1 << 22), ("gzip", 1 << 16), ("gzip", 1 << 20)]:
        out = str(inputs["tmp"] / ("out_%s_%d.cmh" % (form, batch)))
        assert hpgv.run_assoc_cmh(inputs["paths"][form], inputs["ped"], inputs["within"], out, batch) == (N_RECORDS, expected[1], expected[2])
        files.append(open(out, "rb").read())
        assert files[-1].split(b"\n") == expected[0].split(b"\n")
    assert all(f == files[0] for f in files)
    assert b"\t3\tnan\tnan\tnan\tnan\tnan\tnan\tnan\tnan\n" in files[0]      # the monomorphic record: three strata take part, every number nan
    assert expected[1] == int((inputs["pheno"] != 0).sum()) - 1      # the sample without a line left the cohort


def test_one_stratum_for_everyone_is_the_chisq_file(inputs):
    tmp = inputs["tmp"]
    out, chisq = str(tmp / "one.cmh"), str(tmp / "plain.chisq")
    n_cohort = int((inputs["pheno"] != 0).sum())
    assert hpgv.run_assoc_cmh(inputs["paths"]["plain"], inputs["ped"], inputs["one"], out) == (N_RECORDS, n_cohort, 1)
    hpgv.build()
    H = C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)
    H.hpgv_run_assoc.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long)]
    n = C.c_long(0)
    assert H.hpgv_run_assoc(inputs["paths"]["plain"].encode(), inputs["ped"].encode(), chisq.encode(), hpgv.TASK_CHISQ, 1 << 22, C.byref(n)) == 0
    cmh = [l.split("\t") for l in open(out).read().splitlines()[1:]]
    ref = [l.split("\t") for l in open(chisq).read().splitlines()[1:]]
    assert [l[:3] for l in cmh] == [l[:3] for l in ref] and len(cmh) == N_RECORDS
    checked = 0
    for c, r in zip(cmh, ref):
        if c[0] == "X":
            continue
        a1, u1, a2, u2 = int(r[4]), int(r[5]), int(r[9]), int(r[10])             # C_A1 C_U1 .. C_A2 C_U2 of the .chisq line
        total = a1 + u1 + a2 + u2
        got, want = float(c[6]), float(r[14]) * (total - 1) / total
        # both files print six decimals: each side is off by at most 5e-7
        assert (got != got and want != want) or abs(got - want) <= 1.1e-6, (c, r)
        checked += got == got
    assert checked >= N_RECORDS // 2
    # and the file itself is the oracle's for that stratification
    recs = _records(inputs, np.where(inputs["pheno"] != 0, 0, -1).astype(np.int32), 1)
    want = open(out).read().splitlines()[1:]
    assert sorted(want) == sorted(cg.format_line(chrom, pos, vid, "A", "C", r) for (chrom, pos, vid, _), r in zip(inputs["rows"], recs))
