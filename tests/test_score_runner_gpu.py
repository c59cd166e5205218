"""hpgv_run_score: the allele-scoring runner.  Its .profile is, line for line, what a Python writer makes of the numpy golden of the
whole VCF and the score file -- whatever the batch size, the input form and the number of devices --, its counters are the
golden's, a bad score file writes nothing, and the file goes into hpgv_run_assoc_logistic as its covariates."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import model_golden as mg
import score_golden as sg
from helpers import hpgv, random_codes
from test_host_logic_cpu import _bgzf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, NV, K = 70, 400, 3                                           # 120 KB of text: two batches of the smallest size
SCORE_NAMES = ["PC1", "PRS", "BURDEN"]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    hpgv.build()
    tmp = tmp_path_factory.mktemp("score_runner")
    rng = np.random.default_rng(47)
    codes = random_codes(rng, NV, NS, quirks=False, strict=False, p_missing=0.04)
    codes[:, 16] = 0xFF                                          # a sample without a call
    v = np.arange(NV)
    multi = v % 23 == 5                                          # ALT "C,G"
    no_id = v % 19 == 3                                          # ID "."
    on_x = v % 17 == 2
    ref_named = (v % 2 == 1)                                     # half the file's alleles name REF
    absent = v % 29 == 7                                         # records the score file does not name
    neither = v % 31 == 11                                       # the file's allele is neither REF nor ALT
    names = ["S%02d" % j for j in range(NS)]
    lines = mg.text_of(codes).split(b"\n")[:-1]
    body = []
    for i, l in enumerate(lines):
        f = l.split(b"\t", 5)
        f[0] = b"X" if on_x[i] else (b"1" if i < 150 else b"2")
        f[2] = b"." if no_id[i] else b"rs%d" % i
        f[3], f[4] = b"A", (b"C,G" if multi[i] else b"C")
        body.append(b"\t".join(f) + b"\n")
    body = b"".join(body)
    head = ("##fileformat=VCFv4.1\n##source=test\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n").encode()
    paths = dict(plain=str(tmp / "in.vcf"), gzip=str(tmp / "in_gz.vcf.gz"), bgzip=str(tmp / "in_bgz.vcf.gz"))
    open(paths["plain"], "wb").write(head + body)
    open(paths["gzip"], "wb").write(gzip.compress(head + body))
    open(paths["bgzip"], "wb").write(_bgzf(head + body, 0x4000))
    assert len(body) > (1 << 16)
    # the score file: a header, three columns of different magnitudes, lines in another order than the VCF's, ids the VCF lacks
    w = np.stack([rng.standard_normal(NV) * 0.05, rng.standard_normal(NV) * 300.0, rng.integers(0, 2, NV).astype(np.float64)], axis=1)
    text_w = [["%.10g" % x for x in row] for row in w]
    w = np.array([[float(x) for x in row] for row in text_w])    # the weights as the file holds them
    score = str(tmp / "weights.txt")
    with open(score, "w") as f:
        f.write("ID A1 %s\n" % " ".join(SCORE_NAMES))
        for i in rng.permutation(NV):
            if absent[i]:
                continue
            allele = "T" if neither[i] else ("A" if ref_named[i] else "C")
            f.write("rs%d\t%s  %s\n" % (i, allele, " ".join(text_w[i])))
        for extra in (100000, 100001, 100002):
            f.write("rs%d C 1 2 3\n" % extra)
        f.write(". C 1 2 3\n")                                    # no record with the id "." ever matches
    in_file = ~absent
    s = np.array([hpgv.score_frac_bits(np.abs(np.concatenate([w[in_file, k], [1.0 + k]])).max()) for k in range(K)], np.int32)
    takes_part = in_file & ~multi & ~no_id & ~neither
    flags = np.where(takes_part, np.where(ref_named, sg.FLIP, 0), sg.SKIP).astype(np.uint8)
    n_unmatched = int((in_file & ~multi & ~no_id & neither).sum())
    G = {imp: sg.golden(codes, w, s, flags, imp, on_x.astype(np.uint8)) for imp in (0, 1)}
    assert 200 < G[1]["const"][K] < NV - 60 and n_unmatched >= 5 and (flags[G[1]["used"]] == sg.FLIP).sum() > 80
    text = {imp: sg.profile_text(names, SCORE_NAMES, G[imp]["acc"], G[imp]["const"], s, imp) for imp in (0, 1)}
    return dict(tmp=tmp, paths=paths, score=score, golden=G, text=text, n_unmatched=n_unmatched, names=names, s=s)


def test_the_golden_is_a_score(inputs):
    """what the comparisons below compare against: the burden column counts alleles, the sample without a call has no average
    without imputation and the cohort's mean with it"""
    G, s = inputs["golden"], inputs["s"]
    val = sg.value(G[0]["acc"], G[0]["const"], s)
    assert (val[2] == np.rint(val[2])).all() and val[2].max() > 20 and val[:, 16].tolist() == [0.0, 0.0, 0.0]
    lines = inputs["text"][0].split("\n")
    assert lines[0] == "#FID\tIID\tCNT\tCNT2\tPC1_SUM\tPC1_AVG\tPRS_SUM\tPRS_AVG\tBURDEN_SUM\tBURDEN_AVG" and len(lines) == NS + 2
    assert lines[17].split("\t")[:4] == ["S16", "S16", "0", "0"] and lines[17].split("\t")[5] == "nan"
    assert inputs["text"][1].split("\n")[17].split("\t")[2] == str(2 * int(G[1]["const"][K])) and "nan" not in inputs["text"][1]


@pytest.mark.parametrize("form,batch", [("plain", 1 << 16), ("plain", 1 << 22), ("gzip", 1 << 16), ("bgzip", 1 << 16), ("bgzip", 1 << 22)])
def test_the_profile_is_the_golden_writers(inputs, form, batch):
    out = str(inputs["tmp"] / ("out_%s_%d.profile" % (form, batch)))
    n, ns, u = hpgv.run_score(inputs["paths"][form], inputs["score"], out, True, batch)
    assert (n, ns, u) == (int(inputs["golden"][1]["const"][K]), NS, inputs["n_unmatched"])
    got = open(out).read()
    for a, b in zip(got.split("\n"), inputs["text"][1].split("\n")):
        assert a == b
    assert got == inputs["text"][1]


def test_without_imputation(inputs):
    out = str(inputs["tmp"] / "noimp.profile")
    n, ns, u = hpgv.run_score(inputs["paths"]["plain"], inputs["score"], out, False, 1 << 16)
    assert (n, ns, u) == (int(inputs["golden"][0]["const"][K]), NS, inputs["n_unmatched"])
    got = open(out).read()
    assert got == inputs["text"][0] and got != inputs["text"][1]
    rows0 = [l.split("\t") for l in got.split("\n")[1:-1]]
    rows1 = [l.split("\t") for l in inputs["text"][1].split("\n")[1:-1]]
    # the averages change (another denominator, and no imputed terms); the sample without a call: every byte missing, half the
    # rows flipped, and exactly 0
    assert all(a[5] != b[5] for a, b in zip(rows0, rows1)) and rows0[16][4:] == ["0", "nan"] * K


_RUNNER = """
import importlib, sys
sys.path.insert(0, %(root)r)
h = importlib.import_module("hpg-variant_amd")
print(*h.run_score(sys.argv[1], sys.argv[2], sys.argv[3], True, 1 << 16))
"""


def test_two_devices_write_the_same_file(inputs):
    """HPGV_DEVICES=0,0: two contexts on the one GPU, a buffer of sums each, added when the run ends"""
    script = inputs["tmp"] / "run.py"
    script.write_text(_RUNNER % {"root": ROOT})
    out = str(inputs["tmp"] / "two.profile")
    env = dict(os.environ, HPGV_DEVICES="0,0")
    r = subprocess.run([sys.executable, str(script), inputs["paths"]["bgzip"], inputs["score"], out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(int(inputs["golden"][1]["const"][K])), str(NS), str(inputs["n_unmatched"])]
    assert open(out).read() == inputs["text"][1]


def test_a_bad_score_file_writes_nothing(inputs):
    tmp, vcf = inputs["tmp"], inputs["paths"]["plain"]
    out = str(tmp / "refused.profile")
    bad = dict(ragged="rs1 C 1 2\nrs2 C 1\n", ragged_header="ID A1 X Y\nrs1 C 1\n", text="rs1 C 1\nrs2 C abc\n", tail="rs1 C 1x\n", nan="rs1 C nan\n",
               inf="rs1 C 1\nrs2 C -inf\n", huge="rs1 C 1e999\n", dup="rs1 C 1\nrs2 C 2\nrs1 A 3\n", wide="rs1 C " + " ".join(["1"] * 33) + "\n",
               narrow="rs1 C\n", empty="", header_only="ID A1 X\n")
    for name, text in bad.items():
        path = str(tmp / ("bad_%s.txt" % name))
        open(path, "w").write(text)
        with pytest.raises(hpgv.HpgvError) as e:
            hpgv.run_score(vcf, path, out)
        assert e.value.code == hpgv.ERR_INVALID, name
    for v, sc, o in ((None, inputs["score"], out), (vcf, None, out), (vcf, inputs["score"], None), (vcf, str(tmp / "missing.txt"), out)):
        with pytest.raises(hpgv.HpgvError) as e:
            hpgv.run_score(v, sc, o)
        assert e.value.code == hpgv.ERR_INVALID
    with pytest.raises(hpgv.HpgvError):
        hpgv.run_score(str(tmp / "missing.vcf"), inputs["score"], out)
    assert not os.path.exists(out)
    # 32 columns are taken, and a file without a header names them SCORE1 ..
    path = str(tmp / "wide_ok.txt")
    open(path, "w").write("rs1 C " + " ".join(str(k + 1) for k in range(32)) + "\nrs4 A " + " ".join(["0.5"] * 32) + "\n")
    out32 = str(tmp / "wide_ok.profile")
    n, ns, u = hpgv.run_score(vcf, path, out32)
    head = open(out32).readline().rstrip("\n").split("\t")
    assert (n, ns, u) == (2, NS, 0) and head[4:6] == ["SCORE1_SUM", "SCORE1_AVG"] and head[-1] == "SCORE32_AVG" and len(head) == 4 + 64


def test_the_profile_goes_in_as_covariates(inputs):
    """the projection use, end to end: the .profile (written without imputation, so that CNT varies) is hpgv_run_assoc_logistic's
    covar_path -- its header is taken by the reader's #FID rule -- and the run uses its first three value columns"""
    tmp, names = inputs["tmp"], inputs["names"]
    prof = str(tmp / "covar.profile")
    hpgv.run_score(inputs["paths"]["plain"], inputs["score"], prof, False)
    rng = np.random.default_rng(3)
    pheno = rng.choice([1, 2], NS)
    ped = str(tmp / "ped.txt")
    with open(ped, "w") as f:
        for k in range(NS):
            f.write("fam%d %s 0 0 %d %d\n" % (k, names[k], 1 + k % 2, pheno[k]))
    cov, have = hpgv.covar_read(prof, names, 3)
    rows = [l.split("\t") for l in open(prof).read().split("\n")[1:-1]]
    assert have.all() and cov.shape[1] >= 3 and np.array_equal(cov[:, :3], np.array([[float(x) for x in r[2:5]] for r in rows]))
    out = str(tmp / "logistic.txt")
    n, used = hpgv.run_assoc_logistic(inputs["paths"]["plain"], ped, prof, out, 3)
    assert used == NS and n > 300
    body = [l.split("\t") for l in open(out).read().split("\n")[1:-1]]
    assert len(body) == n and sum(r[10] != "nan" for r in body) > n // 2      # fits with the three covariates converge
    # (the AVG columns hold a nan for the sample without a call: all of the file's columns in use would drop that sample)
    assert hpgv.run_assoc_logistic(inputs["paths"]["plain"], ped, prof, out, 4)[1] == NS - 1
