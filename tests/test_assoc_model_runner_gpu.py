"""hpgv_run_assoc_model: the model tests' file runner.  Its result file is what the Python path (Engine.assoc_model_text over the
whole file in one call) formats, line by line; its .mperm file is what perm_labels_shuffle + assoc_model_text + perm_pvalues give
over the whole file, whatever the batch size and the input form (plain, gzip, bgzip)."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from helpers import hpgv
from oracle import pyoracle as orc
from test_host_logic_cpu import _bgzf
from test_host_mirror_gpu import _write_inputs

pytestmark = pytest.mark.gpu

N_PERMS, SEED = 50, 20240611
HEADER = "#CHR\tPOS\tID\tA1\tA2\tAFF\tUNAFF\tCHISQ_GENO\tP_GENO\tCHISQ_TREND\tP_TREND\tCHISQ_ALLELIC\tP_ALLELIC\tCHISQ_DOM\tP_DOM\tCHISQ_REC\tP_REC\n"


@pytest.fixture(scope="module")
def host():
    hpgv.build()
    from importlib import import_module
    b = import_module("hpg-variant_amd._build")
    L = C.CDLL(b.HOSTLIB)
    L.hpgv_host_format_f6.argtypes = [C.c_double, C.c_char_p]
    yield L
    L.hpgv_host_shutdown()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("model_runner")
    rng = np.random.default_rng(23)
    people, names, rows = _write_inputs(tmp, rng, 12, 30, 300)
    head = "##fileformat=VCFv4.1\n##source=test\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n"
    body = "".join("%s\t%d\trs%d\tA\tC\t.\tPASS\t.\t%s\t%s\n" % (chrom, 1000 + v, v, fmt, "\t".join(samples))
                   for v, (chrom, fmt, samples) in enumerate(rows))
    paths = dict(plain=str(tmp / "in.vcf"), gzip=str(tmp / "in_gz.vcf.gz"), bgzip=str(tmp / "in_bgz.vcf.gz"))
    data = (head + body).encode()
    open(paths["plain"], "wb").write(data)
    open(paths["gzip"], "wb").write(gzip.compress(data))
    open(paths["bgzip"], "wb").write(_bgzf(data, 0x4000))
    pheno = {p[1]: p[5] for p in people}
    cond = np.array([{2: orc.AFFECTED, 1: orc.UNAFFECTED}.get(pheno[n], orc.COND_OTHER) for n in names], np.uint8)
    return dict(tmp=tmp, paths=paths, ped=str(tmp / "ped.txt"), rows=rows, cond=cond, body=body.encode())


def _f6(host, x):
    buf = C.create_string_buffer(320)
    n = host.hpgv_host_format_f6(float(x), buf)
    return buf.raw[:n].decode()


def _sorted(path):
    return subprocess.run(["sort", "-k1,1h", "-k2,2n", str(path)], capture_output=True, env=dict(os.environ, LC_ALL="C"), check=True).stdout


@pytest.fixture(scope="module")
def expected_of(host, inputs):
    """n_perms -> the two files from the Python path over the whole file in one call"""
    made = {}

    def of(n_perms):
        if n_perms not in made:
            made[n_perms] = _expected(host, inputs, n_perms)
        return made[n_perms]
    return of


@pytest.fixture(scope="module")
def expected(expected_of):
    return expected_of(N_PERMS)


def _expected(host, inputs, n_perms):
    tmp, rows = inputs["tmp"], inputs["rows"]
    e = hpgv.Engine(0)
    e.set_cohort(inputs["cond"])
    e.set_perm_labels(hpgv.perm_labels_shuffle(inputs["cond"], n_perms, SEED))
    res = e.assoc_model_text(inputs["body"], perm=True)
    e.close()
    assert res["n_lines"] == len(rows) and not res["status"].any()
    t_obs = np.ascontiguousarray(res["chisq5"][:, hpgv.MODEL_TREND])
    emp1, emp2 = hpgv.perm_pvalues(t_obs, res["n_ge"], res["batch_max"])
    # the comparisons below say something: most rows have a statistic, and the p-values vary from row to row
    assert np.isfinite(emp2).sum() > 200 and len(set(emp1[np.isfinite(emp1)])) > 5 and len(set(emp2[np.isfinite(emp2)])) > 1
    model, mperm = tmp / ("expected_%d.model" % n_perms), tmp / ("expected_%d.mperm" % n_perms)
    with open(model, "w") as f, open(mperm, "w") as g:
        f.write(HEADER)
        g.write("#CHR\tPOS\tID\tEMP1\tEMP2\n")
        for v, (chrom, _, _) in enumerate(rows):
            c = res["counts8"][v]
            stats = "\t".join("%s\t%s" % (_f6(host, res["chisq5"][v, t]), _f6(host, res["p5"][v, t])) for t in range(5))
            f.write("%s\t%d\trs%d\tA\tC\t%d/%d/%d\t%d/%d/%d\t%s\n" % (chrom, 1000 + v, v, c[0], c[1], c[2], c[3], c[4], c[5], stats))
            g.write("%s\t%d\trs%d\t%s\t%s\n" % (chrom, 1000 + v, v, _f6(host, emp1[v]), _f6(host, emp2[v])))
    return _sorted(model), _sorted(mperm)


@pytest.mark.parametrize("form", ["plain", "gzip", "bgzip"])
@pytest.mark.parametrize("batch", [1 << 16, 1 << 22])
@pytest.mark.parametrize("n_perms", [N_PERMS, 150])      # one pass of the permutation kernel; two
def test_model_file_and_mperm(inputs, expected_of, form, batch, n_perms):
    expected = expected_of(n_perms)
    out = str(inputs["tmp"] / ("perm_%s_%d_%d.model" % (form, batch, n_perms)))
    n = hpgv.run_assoc_model(inputs["paths"][form], inputs["ped"], out, n_perms, SEED, batch)
    assert n == len(inputs["rows"])
    got = open(out, "rb").read()
    assert got.split(b"\n") == expected[0].split(b"\n")
    assert open(out + ".mperm", "rb").read() == expected[1]
    assert os.path.getsize(inputs["paths"]["plain"]) > (1 << 16)        # the 64 KiB runs are several batches


def test_the_seed_fixes_the_file_and_no_permutations_write_no_mperm(inputs, expected):
    tmp = inputs["tmp"]
    a, b, c = (str(tmp / ("seed_%s.model" % k)) for k in "abc")
    hpgv.run_assoc_model(inputs["paths"]["plain"], inputs["ped"], a, N_PERMS, SEED, 1 << 16)
    hpgv.run_assoc_model(inputs["paths"]["plain"], inputs["ped"], b, N_PERMS, SEED, 1 << 18)
    hpgv.run_assoc_model(inputs["paths"]["plain"], inputs["ped"], c, N_PERMS, SEED + 1, 1 << 16)
    assert open(a + ".mperm", "rb").read() == open(b + ".mperm", "rb").read() == expected[1]
    assert open(c + ".mperm", "rb").read() != expected[1]
    assert open(c, "rb").read() == expected[0]
    none = str(tmp / "none.model")
    assert hpgv.run_assoc_model(inputs["paths"]["plain"], inputs["ped"], none, 0, SEED, 1 << 16) == len(inputs["rows"])
    assert open(none, "rb").read() == expected[0] and not os.path.exists(none + ".mperm")
