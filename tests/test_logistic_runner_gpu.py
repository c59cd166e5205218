"""hpgv_run_assoc_logistic: the logistic regression's file runner.  Its file is the numpy oracle's fit of every record, formatted
line by line, with 3 covariates and, on a second cohort, with 10 and with the first 6 of 10 (k_logistic<12,2> and <8,1>); the bytes
do not depend on the batch size or the input form; a sample without covariates leaves the cohort; the
.eigenvec file of hpgv_run_pca is a covariate file as it stands; what is refused before the engine starts writes no file."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import logistic_golden as lg
from helpers import hpgv
from test_host_logic_cpu import _bgzf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "#CHR\tPOS\tID\tA1\tA2\tNOBS\tBETA\tSE\tOR\tSTAT\tP\tITER\n"
N_SAMPLES, N_RECORDS, N_COV = 60, 40, 3


def _make_inputs(tmp, seed, n_samples, n_records, n_cov):
    rng = np.random.default_rng(seed)
    names = ["S%d" % i for i in rng.permutation(n_samples)]
    pheno = rng.choice([1, 2, 2, 1, 0], n_samples)                   # 0: in no class
    with open(tmp / "ped.txt", "w") as f:
        for k in rng.permutation(n_samples):                         # PED order is not the VCF's
            f.write("fam%d %s 0 0 %d %d\n" % (k, names[k], 1 + k % 2, pheno[k]))
    cov = rng.standard_normal((n_samples, n_cov))
    cohort = np.flatnonzero(pheno != 0)
    absent, na = int(cohort[4]), int(cohort[9])                      # one cohort sample without a line, one with NA in the last column
    with open(tmp / "covar.txt", "w") as f:
        f.write("FID IID %s\n" % " ".join("PC%d" % (k + 1) for k in range(n_cov)))
        for k in rng.permutation(n_samples):
            if k == absent:
                continue
            vals = ["%.17g" % x for x in cov[k]]
            if k == na:
                vals[n_cov - 1] = "NA"
            f.write("fam%d\t%s  %s\n" % (k, names[k], " ".join(vals)))
        f.write("famX nobody %s\n" % " ".join(str(k + 1) for k in range(n_cov)))      # a line of a sample the VCF does not have
    gts = np.array(["0/0", "0/1", "1/0", "1/1", "./."])
    rows, lines = [], []
    for v in range(n_records):
        chrom = ("1", "X", "22", "3")[v % 4]
        g = gts[rng.choice(5, n_samples, p=[0.3, 0.2, 0.2, 0.25, 0.05])]
        if v == 7:
            g[:] = "0/0"                                              # monomorphic: a failed fit in the file
        cls = np.array([{"0/0": 0, "0/1": 1, "1/0": 1, "1/1": 2, "./.": 255}[x] for x in g], np.uint8)
        rows.append((chrom, 5000 - 13 * v, "rs%d" % v, cls))          # positions fall: the file is sorted afterwards
        lines.append("%s\t%d\trs%d\tA\tC\t.\tPASS\t.\tGT\t%s\n" % (chrom, 5000 - 13 * v, v, "\t".join(g)))
    head = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n"
    data = (head + "".join(lines)).encode()
    paths = dict(plain=str(tmp / "in.vcf"), gzip=str(tmp / "in_gz.vcf.gz"), bgzip=str(tmp / "in_bgz.vcf.gz"))
    open(paths["plain"], "wb").write(data)
    open(paths["gzip"], "wb").write(gzip.compress(data))
    open(paths["bgzip"], "wb").write(_bgzf(data, 0x1000))
    return dict(tmp=tmp, paths=paths, ped=str(tmp / "ped.txt"), covar=str(tmp / "covar.txt"), names=names, pheno=pheno, cov=cov, rows=rows,
                absent=absent, na=na, n_data_bytes=len("".join(lines)))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return _make_inputs(tmp_path_factory.mktemp("logistic_runner"), 77, N_SAMPLES, N_RECORDS, N_COV)


# ten covariate columns, as the ten principal components of a .eigenvec file: all of them -> p = 12, k_logistic<12,2>; the first six
# -> p = 8, k_logistic<8,1>.  About 125 of the 170 samples are in a class: more than ten observations per coefficient.  The
# records fill more than one batch of the smallest size (64 KiB).
WIDE_SAMPLES, WIDE_RECORDS, WIDE_COV = 170, 110, 10


@pytest.fixture(scope="module")
def wide_inputs(tmp_path_factory):
    w = _make_inputs(tmp_path_factory.mktemp("logistic_runner_wide"), 78, WIDE_SAMPLES, WIDE_RECORDS, WIDE_COV)
    assert w["n_data_bytes"] > (1 << 16) and (w["pheno"] != 0).sum() - 2 >= 10 * (WIDE_COV + 2)
    return w


def _sorted(text):
    return subprocess.run(["sort", "-k1,1h", "-k2,2n"], input=text.encode(), capture_output=True, env=dict(os.environ, LC_ALL="C"), check=True).stdout


def _expected(inputs, used, cov):
    """the oracle's file for the cohort samples `used` (a mask) and their covariates"""
    y = (inputs["pheno"][used] == 2).astype(np.uint8)
    out, n_ok = [HEADER], 0
    for chrom, pos, vid, cls in inputs["rows"]:
        r = lg.fit(cls[used], y, cov[used] if cov is not None else None)
        n_ok += r["status"] == lg.OK
        out.append(lg.format_line(chrom, pos, vid, "A", "C", r) + "\n")
    assert n_ok >= len(inputs["rows"]) - 2                            # the comparison says something
    return _sorted("".join(out))


@pytest.fixture(scope="module")
def expected(inputs):
    used = inputs["pheno"] != 0
    used[[inputs["absent"], inputs["na"]]] = False
    return _expected(inputs, used, inputs["cov"]), int(used.sum())


@pytest.mark.parametrize("form,batch", [("plain", 1 << 16), ("plain", 1 << 22), ("bgzip", 1 << 16), ("gzip", 1 << 20)])
def test_the_file_is_the_oracles(inputs, expected, form, batch):
    out = str(inputs["tmp"] / ("out_%s_%d.logistic" % (form, batch)))
    n, used = hpgv.run_assoc_logistic(inputs["paths"][form], inputs["ped"], inputs["covar"], out, 0, batch)
    assert (n, used) == (N_RECORDS, expected[1])
    got = open(out, "rb").read()
    assert got.split(b"\n") == expected[0].split(b"\n")
    assert b"\tnan\tnan\tnan\tnan\tnan\t0\n" in got                   # the monomorphic record: five nan, no step


@pytest.mark.parametrize("n_covar", [0, 6], ids=["all_10_columns", "first_6_columns"])
def test_the_file_with_ten_and_with_six_covariates_is_the_oracles(wide_inputs, n_covar):
    """k_logistic<12,2> and <8,1> through the runner: line by line the oracle's, the same bytes whatever the batch size"""
    w = wide_inputs
    used = w["pheno"] != 0
    used[w["absent"]] = False
    if n_covar == 0:
        used[w["na"]] = False                                         # the NA is in the tenth column
    want = _expected(w, used, w["cov"][:, :n_covar or WIDE_COV])
    files = []
    for batch in (1 << 16, 1 << 22):                                  # two batches, one batch
        out = str(w["tmp"] / ("out_%d_%d.logistic" % (n_covar, batch)))
        assert hpgv.run_assoc_logistic(w["paths"]["plain"], w["ped"], w["covar"], out, n_covar, batch) == (WIDE_RECORDS, int(used.sum()))
        files.append(open(out, "rb").read())
        assert files[-1].split(b"\n") == want.split(b"\n")
    assert files[0] == files[1]
    assert files[0].count(b"\tnan\tnan\tnan\tnan\tnan\t") == 1      # the monomorphic record alone failed


def test_a_sample_without_covariates_leaves_the_cohort_only_where_the_column_is_used(inputs, expected):
    tmp = inputs["tmp"]
    used = inputs["pheno"] != 0
    used[inputs["absent"]] = False                                   # two columns in use: the NA is in the third
    two = str(tmp / "two.logistic")
    assert hpgv.run_assoc_logistic(inputs["paths"]["plain"], inputs["ped"], inputs["covar"], two, 2) == (N_RECORDS, int(used.sum()))
    assert open(two, "rb").read() == _expected(inputs, used, inputs["cov"][:, :2])
    none = str(tmp / "none.logistic")                                # no file: no covariates, the whole cohort
    whole = inputs["pheno"] != 0
    assert hpgv.run_assoc_logistic(inputs["paths"]["plain"], inputs["ped"], None, none) == (N_RECORDS, int(whole.sum()))
    assert open(none, "rb").read() == _expected(inputs, whole, None)
    assert open(none, "rb").read() != expected[0]


def test_the_eigenvec_file_of_the_pca_run_is_a_covariate_file(inputs):
    tmp = inputs["tmp"]
    prefix = str(tmp / "pcs")
    hpgv.run_pca(inputs["paths"]["plain"], prefix, 0.01, 3)
    table = [l.split("\t") for l in open(prefix + ".eigenvec").read().splitlines()]
    assert [t[1] for t in table] == inputs["names"] and len(table[0]) == 5
    cov = np.array([[float(x) for x in t[2:4]] for t in table])
    out = str(tmp / "pcs.logistic")
    whole = inputs["pheno"] != 0
    assert hpgv.run_assoc_logistic(inputs["paths"]["plain"], inputs["ped"], prefix + ".eigenvec", out, 2) == (N_RECORDS, int(whole.sum()))
    assert open(out, "rb").read() == _expected(inputs, whole, cov)


_RUNNER = """
import importlib, sys
sys.path.insert(0, %(root)r)
h = importlib.import_module("hpg-variant_amd")
print(*h.run_assoc_logistic(sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], 0, 1 << 16))
"""


def test_two_devices_write_the_same_file(inputs, expected):
    """HPGV_DEVICES=0,0: two contexts on the one GPU, the covariates on both, the batches dealt to them"""
    script = inputs["tmp"] / "run.py"
    script.write_text(_RUNNER % {"root": ROOT})
    out = str(inputs["tmp"] / "two_devices.logistic")
    env = dict(os.environ, HPGV_DEVICES="0,0")
    r = subprocess.run([sys.executable, str(script), inputs["paths"]["bgzip"], inputs["ped"], inputs["covar"], out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(N_RECORDS), str(expected[1])]
    assert open(out, "rb").read() == expected[0]


def test_what_is_refused_before_the_engine_starts_writes_no_file(inputs):
    tmp, vcf, ped, covar = inputs["tmp"], inputs["paths"]["plain"], inputs["ped"], inputs["covar"]
    bad = {}
    for name, text in [("dup", "a S1 1 2\nb S1 3 4\n"), ("ragged", "a S1 1 2\na S2 3\n"), ("wide", "a S1 " + " ".join(["1"] * 15) + "\n")]:
        bad[name] = str(tmp / ("bad_%s.txt" % name))
        open(bad[name], "w").write(text)
    out = str(tmp / "refused.logistic")
    calls = [(None, ped, covar, out, 0), (vcf, None, covar, out, 0), (vcf, ped, covar, None, 0), (vcf, ped, bad["dup"], out, 0),
             (vcf, ped, bad["ragged"], out, 0), (vcf, ped, bad["wide"], out, 0), (vcf, ped, str(tmp / "missing.txt"), out, 0),
             (vcf, ped, covar, out, -1), (vcf, ped, covar, out, 4), (vcf, ped, covar, out, 15), (vcf, ped, None, out, 2)]
    for args in calls:
        with pytest.raises(hpgv.HpgvError) as err:
            hpgv.run_assoc_logistic(*args)
        assert err.value.code == hpgv.ERR_INVALID, args
        assert not os.path.exists(out), args
    assert hpgv.run_assoc_logistic(vcf, ped, bad["wide"], out, 14)[0] == N_RECORDS      # 15 columns, 14 in use
