"""hpgv_run_assoc_linear: the linear regression's file runner.  Its file is the extended-precision oracle's fit of every record,
formatted line by line; the bytes do not depend on the batch size or the input form; a sample whose trait is -9 or no number, or
that has no covariate line, leaves the cohort; the trait may come from a phenotype file instead of the PED; the .eigenvec file of
hpgv_run_pca is a covariate file as it stands; what is refused before the engine starts writes no file."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import linear_golden as ln
from helpers import hpgv
from test_host_logic_cpu import _bgzf

pytestmark = pytest.mark.gpu

HEADER = "#CHR\tPOS\tID\tA1\tA2\tNOBS\tBETA\tSE\tSTAT\tP\n"
N_SAMPLES, N_RECORDS, N_COV = 60, 40, 3


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("linear_runner")
    rng = np.random.default_rng(78)
    names = ["S%d" % i for i in rng.permutation(N_SAMPLES)]
    trait = np.array([float("%.3f" % x) for x in 170.0 + 8.0 * rng.standard_normal(N_SAMPLES)])     # what the files' tokens read as
    trait5 = np.array([float("%.3f" % (x + 5.0)) for x in trait])
    minus9, na, absent, cov_na = 5, 11, 17, 23                       # trait -9, trait NA, no covariate line, NA in the last covariate
    token = ["%.3f" % x for x in trait]
    token[minus9], token[na] = "-9", "NA"
    with open(tmp / "ped.txt", "w") as f:
        for k in rng.permutation(N_SAMPLES):                         # PED order is not the VCF's
            f.write("fam%d %s 0 0 %d %s\n" % (k, names[k], 1 + k % 2, token[k]))
    with open(tmp / "pheno.txt", "w") as f:                          # the same trait shifted by 5, as a file; a second column that is not used
        f.write("FID IID height other\n")
        for k in rng.permutation(N_SAMPLES):
            if k != absent + 1:
                f.write("fam%d %s %s 1\n" % (k, names[k], "NA" if k in (minus9, na) else "%.3f" % trait5[k]))
    cov = rng.standard_normal((N_SAMPLES, N_COV))
    with open(tmp / "covar.txt", "w") as f:
        f.write("FID IID PC1 PC2 PC3\n")
        for k in rng.permutation(N_SAMPLES):
            if k == absent:
                continue
            vals = ["%.17g" % x for x in cov[k]]
            if k == cov_na:
                vals[2] = "NA"
            f.write("fam%d\t%s  %s\n" % (k, names[k], " ".join(vals)))
        f.write("famX nobody 1 2 3\n")                               # a line of a sample the VCF does not have
    gts = np.array(["0/0", "0/1", "1/0", "1/1", "./."])
    rows, lines = [], []
    for v in range(N_RECORDS):
        chrom = ("1", "X", "22", "3")[v % 4]
        g = gts[rng.choice(5, N_SAMPLES, p=[0.3, 0.2, 0.2, 0.25, 0.05])]
        if v == 7:
            g[:] = "0/0"                                              # monomorphic: a singular fit in the file
        cls = np.array([{"0/0": 0, "0/1": 1, "1/0": 1, "1/1": 2, "./.": 255}[x] for x in g], np.uint8)
        rows.append((chrom, 5000 - 13 * v, "rs%d" % v, cls))          # positions fall: the file is sorted afterwards
        lines.append("%s\t%d\trs%d\tA\tC\t.\tPASS\t.\tGT\t%s\n" % (chrom, 5000 - 13 * v, v, "\t".join(g)))
    head = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n"
    data = (head + "".join(lines)).encode()
    paths = dict(plain=str(tmp / "in.vcf"), gzip=str(tmp / "in_gz.vcf.gz"), bgzip=str(tmp / "in_bgz.vcf.gz"))
    open(paths["plain"], "wb").write(data)
    open(paths["gzip"], "wb").write(gzip.compress(data))
    open(paths["bgzip"], "wb").write(_bgzf(data, 0x1000))
    has_trait = np.ones(N_SAMPLES, bool)
    has_trait[[minus9, na]] = False
    return dict(tmp=tmp, paths=paths, ped=str(tmp / "ped.txt"), pheno=str(tmp / "pheno.txt"), covar=str(tmp / "covar.txt"), names=names, trait=trait, trait5=trait5,
                cov=cov, rows=rows, has_trait=has_trait, absent=absent, cov_na=cov_na)


def _sorted(text):
    return subprocess.run(["sort", "-k1,1h", "-k2,2n"], input=text.encode(), capture_output=True, env=dict(os.environ, LC_ALL="C"), check=True).stdout


def _expected(inputs, used, cov, trait=None):
    """the oracle's file for the cohort samples `used` (a mask), their trait and their covariates"""
    y = (inputs["trait"] if trait is None else trait)[used]
    out, n_ok = [HEADER], 0
    for chrom, pos, vid, cls in inputs["rows"]:
        r = ln.ref_fit(cls[used], y, cov[used] if cov is not None else None)
        n_ok += r["status"] == ln.OK
        out.append(ln.format_line(chrom, pos, vid, "A", "C", r) + "\n")
    assert n_ok >= N_RECORDS - 2                                      # the comparison says something
    return _sorted("".join(out))


@pytest.fixture(scope="module")
def expected(inputs):
    used = inputs["has_trait"].copy()
    used[[inputs["absent"], inputs["cov_na"]]] = False
    return _expected(inputs, used, inputs["cov"]), int(used.sum())


@pytest.mark.parametrize("form,batch", [("plain", 1 << 16), ("plain", 1 << 22), ("bgzip", 1 << 16), ("gzip", 1 << 20)])
def test_the_file_is_the_oracles(inputs, expected, form, batch):
    out = str(inputs["tmp"] / ("out_%s_%d.linear" % (form, batch)))
    n, used = hpgv.run_assoc_linear(inputs["paths"][form], inputs["ped"], None, inputs["covar"], out, 0, batch)
    assert (n, used) == (N_RECORDS, expected[1]) and used == N_SAMPLES - 4
    got = open(out, "rb").read()
    assert got.split(b"\n") == expected[0].split(b"\n")
    assert b"\tnan\tnan\tnan\tnan\n" in got                           # the monomorphic record


def test_who_leaves_the_cohort(inputs, expected):
    tmp = inputs["tmp"]
    used = inputs["has_trait"].copy()
    used[inputs["absent"]] = False                                   # two columns in use: the NA is in the third
    two = str(tmp / "two.linear")
    assert hpgv.run_assoc_linear(inputs["paths"]["plain"], inputs["ped"], None, inputs["covar"], two, 2) == (N_RECORDS, int(used.sum()))
    assert open(two, "rb").read() == _expected(inputs, used, inputs["cov"][:, :2])
    none = str(tmp / "none.linear")                                  # no covariate file: everyone with a trait
    whole = inputs["has_trait"]
    assert hpgv.run_assoc_linear(inputs["paths"]["plain"], inputs["ped"], None, None, none) == (N_RECORDS, N_SAMPLES - 2)
    assert open(none, "rb").read() == _expected(inputs, whole, None)
    assert open(none, "rb").read() != expected[0]


def test_the_trait_from_a_phenotype_file(inputs):
    tmp = inputs["tmp"]
    used = inputs["has_trait"].copy()
    used[inputs["absent"] + 1] = False                               # the sample the phenotype file does not list
    want = _expected(inputs, used, None, inputs["trait5"])
    for ped in (None, inputs["ped"]):                                # the file wins over the PED's column; no PED is needed
        out = str(tmp / ("pheno_%s.linear" % (ped is None)))
        assert hpgv.run_assoc_linear(inputs["paths"]["bgzip"], ped, inputs["pheno"], None, out) == (N_RECORDS, int(used.sum()))
        assert open(out, "rb").read() == want


def test_the_eigenvec_file_of_the_pca_run_is_a_covariate_file(inputs):
    tmp = inputs["tmp"]
    prefix = str(tmp / "pcs")
    hpgv.run_pca(inputs["paths"]["plain"], prefix, 0.01, 3)
    table = [l.split("\t") for l in open(prefix + ".eigenvec").read().splitlines()]
    assert [t[1] for t in table] == inputs["names"] and len(table[0]) == 5
    cov = np.array([[float(x) for x in t[2:4]] for t in table])
    out = str(tmp / "pcs.linear")
    whole = inputs["has_trait"]
    assert hpgv.run_assoc_linear(inputs["paths"]["plain"], inputs["ped"], None, prefix + ".eigenvec", out, 2) == (N_RECORDS, int(whole.sum()))
    assert open(out, "rb").read() == _expected(inputs, whole, cov)


def test_what_is_refused_before_the_engine_starts_writes_no_file(inputs):
    tmp, vcf, ped, covar, pheno = inputs["tmp"], inputs["paths"]["plain"], inputs["ped"], inputs["covar"], inputs["pheno"]
    bad = {}
    for name, text in [("dup", "a S1 1 2\nb S1 3 4\n"), ("ragged", "a S1 1 2\na S2 3\n"), ("wide", "a S1 " + " ".join(["1"] * 15) + "\n"), ("ids", "a S1\na S2\n")]:
        bad[name] = str(tmp / ("bad_%s.txt" % name))
        open(bad[name], "w").write(text)
    out = str(tmp / "refused.linear")
    calls = [(None, ped, None, covar, out, 0), (vcf, None, None, covar, out, 0), (vcf, ped, None, covar, None, 0), (vcf, ped, None, bad["dup"], out, 0),
             (vcf, ped, None, bad["ragged"], out, 0), (vcf, ped, None, bad["wide"], out, 0), (vcf, ped, None, str(tmp / "missing.txt"), out, 0),
             (vcf, ped, None, covar, out, -1), (vcf, ped, None, covar, out, 4), (vcf, ped, None, covar, out, 15), (vcf, ped, None, None, out, 2),
             (vcf, None, bad["dup"], None, out, 0), (vcf, ped, bad["ragged"], None, out, 0), (vcf, None, bad["ids"], None, out, 0),
             (vcf, None, str(tmp / "missing.txt"), None, out, 0)]
    for args in calls:
        with pytest.raises(hpgv.HpgvError) as err:
            hpgv.run_assoc_linear(*args)
        assert err.value.code == hpgv.ERR_INVALID, args
        assert not os.path.exists(out), args
    assert hpgv.run_assoc_linear(vcf, ped, None, bad["wide"], out, 14)[0] == N_RECORDS      # 15 columns, 14 in use
    assert hpgv.run_assoc_linear(vcf, None, pheno, covar, out, 0) == (N_RECORDS, N_SAMPLES - 5)
