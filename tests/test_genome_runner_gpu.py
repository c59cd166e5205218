"""hpgv_run_genome: the relatedness runner.  Its file is what the golden writer makes of the whole VCF -- numpy pair counts, the
terms added in file order, the genome values in the header's order -- byte for byte, whatever the batch size, the input form and
the number of devices."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ibs_golden as ig
import model_golden as mg
from helpers import hpgv, random_codes
from test_host_logic_cpu import _bgzf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "#IID1\tIID2\tNM\tIBS0\tIBS1\tIBS2\tZ0\tZ1\tZ2\tPI_HAT\tDST\n"
NS, NV = 48, 400                                                 # 87 KB of text: two batches of the smallest size
DUP, PARENT = (3, 40), (8, 30)


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
    tmp = tmp_path_factory.mktemp("genome_runner")
    rng = np.random.default_rng(41)
    codes = random_codes(rng, NV, NS, quirks=False, strict=False, p_missing=0.03)
    codes[rng.random((NV, NS)) < 0.01] = 0x12                    # a few "1/2"
    codes[:, DUP[1]] = codes[:, DUP[0]]                          # one duplicated sample, with other missing genotypes
    codes[rng.random(NV) < 0.1, DUP[1]] = 0xFF
    par = codes[:, PARENT[0]]
    codes[:, PARENT[1]] = np.where(par == 0xFF, 0xFF, (np.minimum(par >> 4, 1) << 4) | rng.integers(0, 2, NV).astype(np.uint8))
    on_x = np.zeros(NV, bool)
    on_x[[0, 5, 199, 200, 399]] = True
    on_x[rng.random(NV) < 0.05] = True
    names = ["S%02d" % j for j in range(NS)]
    lines = mg.text_of(codes).split(b"\n")[:-1]
    chrom = lambda v: b"X" if on_x[v] else (b"1" if v < 150 else b"2")
    body = b"".join(chrom(v) + l[1:] + b"\n" for v, l in enumerate(lines))
    head = ("##fileformat=VCFv4.1\n##source=test\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n").encode()
    paths = dict(plain=str(tmp / "in.vcf"), bgzip=str(tmp / "in_bgz.vcf.gz"))
    open(paths["plain"], "wb").write(head + body)
    open(paths["bgzip"], "wb").write(_bgzf(head + body, 0x4000))
    assert len(body) > (1 << 16)
    skip = on_x.astype(np.uint8)
    counts = ig.pair_counts(codes, skip)
    E, used = ig.expected(ig.class_counts(codes, skip))
    assert used > 300
    gen = ig.genome_all(counts, E)
    return dict(tmp=tmp, paths=paths, names=names, counts=counts, gen=gen, n_records=int((~on_x).sum()))


def _f6(host, x):
    buf = C.create_string_buffer(320)
    n = host.hpgv_host_format_f6(float(x), buf)
    return buf.raw[:n].decode()


def _golden_file(host, inputs, min_pi_hat):
    out = [HEADER]
    names, counts, gen = inputs["names"], inputs["counts"], inputs["gen"]
    for i in range(NS):
        for j in range(i + 1, NS):
            if gen[i, j, 3] >= min_pi_hat:
                out.append("%s\t%s\t%d\t%d\t%d\t%d\t%s\n" % (names[i], names[j], *counts[i, j], "\t".join(_f6(host, x) for x in gen[i, j])))
    return "".join(out).encode()


@pytest.mark.parametrize("form,batch", [("plain", 1 << 16), ("plain", 1 << 22), ("bgzip", 1 << 16)])
def test_the_file_is_the_golden_writers(host, inputs, form, batch):
    """min_pi_hat = -1 keeps every pair: more than the first list holds, so the selection runs twice"""
    out = str(inputs["tmp"] / ("all_%s_%d.genome" % (form, batch)))
    n, k = hpgv.run_genome(inputs["paths"][form], out, -1.0, batch)
    exp = _golden_file(host, inputs, -1.0)
    assert n == inputs["n_records"] and k == NS * (NS - 1) // 2 == exp.count(b"\n") - 1
    assert open(out, "rb").read() == exp


def test_min_pi_hat_filters(host, inputs):
    for thr in (0.05, 0.4, 1.0, 2.0):
        out = str(inputs["tmp"] / ("thr_%g.genome" % thr))
        n, k = hpgv.run_genome(inputs["paths"]["plain"], out, thr, 1 << 16)
        exp = _golden_file(host, inputs, thr)
        got = open(out, "rb").read()
        assert got == exp and k == exp.count(b"\n") - 1 and n == inputs["n_records"], thr
    gen = inputs["gen"]
    assert gen[DUP][3] == 1.0 and gen[DUP][2] == 1.0 and gen[PARENT][3] >= 0.4 and gen[PARENT][0] == 0.0
    lines = open(str(inputs["tmp"] / "thr_0.4.genome")).read().split("\n")
    assert any(l.startswith("S03\tS40\t") and l.endswith("\t1.000000\t1.000000\t1.000000") for l in lines)
    assert any(l.startswith("S08\tS30\t") for l in lines) and len(lines) < 12
    assert open(str(inputs["tmp"] / "thr_2.genome"), "rb").read() == HEADER.encode()


def test_refusals_write_no_file(host, inputs):
    out = str(inputs["tmp"] / "refused.genome")
    for vcf, path, thr in ((None, out, 0.1), (inputs["paths"]["plain"], None, 0.1), (inputs["paths"]["plain"], out, float("nan"))):
        with pytest.raises(hpgv.HpgvError) as e:
            hpgv.run_genome(vcf, path, thr)
        assert e.value.code == hpgv.ERR_INVALID
    assert not os.path.exists(out)
    with pytest.raises(hpgv.HpgvError):
        hpgv.run_genome(str(inputs["tmp"] / "missing.vcf"), out, 0.1)
    assert not os.path.exists(out)


_RUNNER = """
import importlib, sys
sys.path.insert(0, %(root)r)
h = importlib.import_module("hpg-variant_amd")
print(*h.run_genome(sys.argv[1], sys.argv[2], float(sys.argv[3]), 1 << 16))
"""


@pytest.mark.parametrize("form", ["plain", "bgzip"])
def test_two_devices_write_the_same_file(host, inputs, form):
    """HPGV_DEVICES=0,0: two contexts on the one GPU, a counts buffer each, added when the run ends"""
    script = inputs["tmp"] / "run.py"
    script.write_text(_RUNNER % {"root": ROOT})
    out = str(inputs["tmp"] / ("two_%s.genome" % form))
    env = dict(os.environ, HPGV_DEVICES="0,0")
    r = subprocess.run([sys.executable, str(script), inputs["paths"][form], out, "0.05"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    exp = _golden_file(host, inputs, 0.05)
    assert open(out, "rb").read() == exp and r.stdout.split() == [str(inputs["n_records"]), str(exp.count(b"\n") - 1)]
