"""hpgv_run_assoc_perm: the chi-square file runner with max(T) label permutation.  Its result file is hpgv_run_assoc's byte for
byte; its .mperm file is what perm_labels_shuffle + Engine.assoc_perm + perm_pvalues give over the whole file in one call,
whatever the batch size and the input form."""
import ctypes as C
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


@pytest.fixture(scope="module")
def host():
    hpgv.build()
    from importlib import import_module
    b = import_module("hpg-variant_amd._build")
    L = C.CDLL(b.HOSTLIB)
    L.hpgv_run_assoc.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long)]
    L.hpgv_run_assoc_perm.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint64, C.c_size_t, C.POINTER(C.c_long)]
    L.hpgv_host_format_f6.argtypes = [C.c_double, C.c_char_p]
    L.hpgv_host_last_error.restype = C.c_char_p
    yield L
    L.hpgv_host_shutdown()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("perm_runner")
    rng = np.random.default_rng(17)
    people, names, rows = _write_inputs(tmp, rng, 12, 18, 300)
    vcf = str(tmp / "in.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n##source=test\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
        for v, (chrom, fmt, samples) in enumerate(rows):
            f.write("%s\t%d\trs%d\tA\tC\t.\tPASS\t.\t%s\t%s\n" % (chrom, 1000 + v, v, fmt, "\t".join(samples)))
    packed = str(tmp / "in.vcf.gz")
    open(packed, "wb").write(_bgzf(open(vcf, "rb").read(), 0x4000))
    pheno = {p[1]: p[5] for p in people}
    cond = np.array([{2: orc.AFFECTED, 1: orc.UNAFFECTED}.get(pheno[n], orc.COND_OTHER) for n in names], np.uint8)
    codes = np.array([[orc.encode_sample(s, fmt.split(":").index("GT"), True) for s in samples] for _, fmt, samples in rows], np.uint8)
    is_x = np.array([1 if c == "X" else 0 for c, _, _ in rows], np.uint8)
    return dict(tmp=tmp, vcf=vcf, packed=packed, ped=str(tmp / "ped.txt").encode(), rows=rows, cond=cond, codes=codes, is_x=is_x)


def _f6(host, x):
    buf = C.create_string_buffer(320)
    n = host.hpgv_host_format_f6(float(x), buf)
    return buf.raw[:n].decode()


@pytest.mark.parametrize("n_perms", [N_PERMS, 150])      # one pass of the permutation kernel; two
def test_result_file_and_mperm(host, inputs, n_perms):
    tmp, rows = inputs["tmp"], inputs["rows"]
    # the Python path over the whole file in one call
    e = hpgv.Engine(0)
    e.set_cohort(inputs["cond"])
    e.set_perm_labels(hpgv.perm_labels_shuffle(inputs["cond"], n_perms, SEED))
    res = e.assoc_perm(inputs["codes"], inputs["is_x"])
    e.close()
    emp1, emp2 = hpgv.perm_pvalues(res["chisq"], res["n_ge"], res["batch_max"])
    assert np.isfinite(emp2).sum() > 200 and len(set(emp2[np.isfinite(emp2)])) > 5      # the comparison below says something
    exp = tmp / ("expected_%d.mperm" % n_perms)
    with open(exp, "w") as f:
        f.write("#CHR\tPOS\tID\tEMP1\tEMP2\n")
        for v, (chrom, _, _) in enumerate(rows):
            f.write("%s\t%d\trs%d\t%s\t%s\n" % (chrom, 1000 + v, v, _f6(host, emp1[v]), _f6(host, emp2[v])))
    expected = subprocess.run(["sort", "-k1,1h", "-k2,2n", str(exp)], capture_output=True, env=dict(os.environ, LC_ALL="C"), check=True).stdout
    # the chi-square runner's file
    plain = str(tmp / "plain.chisq")
    n = C.c_long(0)
    assert host.hpgv_run_assoc(inputs["vcf"].encode(), inputs["ped"], plain.encode(), 1, 1 << 16, C.byref(n)) == 0, host.hpgv_host_last_error()
    assert n.value == len(rows)
    want = open(plain, "rb").read()
    for tag, path, batch in (("several", inputs["vcf"], 1 << 16), ("one", inputs["vcf"], 1 << 22), ("bgzf", inputs["packed"], 1 << 16)):
        out = str(tmp / ("perm_%s_%d.chisq" % (tag, n_perms)))
        n = C.c_long(0)
        rc = host.hpgv_run_assoc_perm(path.encode(), inputs["ped"], out.encode(), n_perms, SEED, batch, C.byref(n))
        assert rc == 0 and n.value == len(rows), (tag, host.hpgv_host_last_error())
        assert open(out, "rb").read() == want, tag
        assert open(out + ".mperm", "rb").read() == expected, tag
    if os.path.getsize(inputs["vcf"]) <= (1 << 16):
        pytest.fail("the VCF fits one batch of 64 KiB: the several-batches run is not one")


def test_no_permutations_is_refused_and_writes_nothing(host, inputs):
    out = str(inputs["tmp"] / "none.chisq")
    for n_perms in (0, -3):
        assert host.hpgv_run_assoc_perm(inputs["vcf"].encode(), inputs["ped"], out.encode(), n_perms, SEED, 1 << 16, None) == hpgv.ERR_INVALID
    assert host.hpgv_run_assoc_perm(inputs["vcf"].encode(), inputs["ped"], None, N_PERMS, SEED, 1 << 16, None) == hpgv.ERR_INVALID
    assert not os.path.exists(out) and not os.path.exists(out + ".mperm")
