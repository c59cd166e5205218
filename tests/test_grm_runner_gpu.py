"""hpgv_run_grm: the relationship-matrix runner.  Its three files are what the golden writer makes of the whole VCF -- the rows' tables
in the header's order, int64 numpy pair sums, the value in the header's order -- byte for byte, whatever the batch size, the input
form and the number of devices."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grm_golden as gg
import ibs_golden as ig
import model_golden as mg
from helpers import hpgv, random_codes
from test_host_logic_cpu import _bgzf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, NV = 48, 400                                                 # 87 KB of text: two batches of the smallest size
MIN_MAF = 0.05
SUFFIXES = (".grm.bin", ".grm.N.bin", ".grm.id")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    hpgv.build()
    tmp = tmp_path_factory.mktemp("grm_runner")
    rng = np.random.default_rng(43)
    codes = random_codes(rng, NV, NS, quirks=False, strict=False, p_missing=0.03)
    codes[rng.random((NV, NS)) < 0.01] = 0x12                    # a few "1/2"
    codes[:, 40] = codes[:, 3]                                   # one duplicated sample, with other missing genotypes
    codes[rng.random(NV) < 0.1, 40] = 0xFF
    mono = [7, 63, 64, 201]                                      # monomorphic rows, of either allele, one with missing genotypes
    codes[mono[:2]] = 0x00
    codes[mono[2:]] = 0x11
    codes[201, ::5] = 0xFF
    rare = [9, 100, 333]                                         # below min_maf: one, two and four alternate alleles among 96
    codes[rare] = 0x00
    codes[9, 4], codes[100, [4, 30]], codes[333, [1, 2]] = 0x01, 0x01, 0x11
    codes[334] = 0x00                                            # five among 96: just above min_maf
    codes[334, [1, 2, 3]] = (0x11, 0x11, 0x10)
    on_x = np.zeros(NV, bool)
    on_x[[0, 5, 199, 200, 399]] = True
    on_x[rng.random(NV) < 0.05] = True
    on_x[mono + rare + [334]] = False
    names = ["S%02d" % j for j in range(NS)]
    lines = mg.text_of(codes).split(b"\n")[:-1]
    chrom = lambda v: b"X" if on_x[v] else (b"1" if v < 150 else b"2")
    body = b"".join(chrom(v) + l[1:] + b"\n" for v, l in enumerate(lines))
    head = ("##fileformat=VCFv4.1\n##source=test\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n").encode()
    paths = dict(plain=str(tmp / "in.vcf"), bgzip=str(tmp / "in_bgz.vcf.gz"))
    open(paths["plain"], "wb").write(head + body)
    open(paths["bgzip"], "wb").write(_bgzf(head + body, 0x4000))
    assert len(body) > (1 << 16)
    s = hpgv.grm_frac_bits(MIN_MAF)
    assert s == 12
    G = gg.golden(codes, s, MIN_MAF, on_x.astype(np.uint8))
    assert not G["used"][mono + rare].any() and G["used"][334] and 300 < G["used"].sum() < NV - on_x.sum() - 6
    return dict(tmp=tmp, paths=paths, golden=gg.files(G["acc"], s, names), n_used=int(G["used"].sum()), acc=G["acc"], s=s)


def _read(prefix):
    return {sfx: open(prefix + sfx, "rb").read() for sfx in SUFFIXES}


def test_the_golden_is_a_relationship_matrix(inputs):
    """what the byte comparisons below compare against: the diagonal near 1, the duplicate's element near its diagonal"""
    val = gg.value(inputs["acc"], inputs["s"])
    d = np.diag(val)
    assert 0.6 < d.min() and d.max() < 1.6 and abs(val[3, 40] - d[3]) < 0.15
    off = val[np.triu_indices(NS, 1)]
    assert abs(np.median(off)) < 0.05
    assert len(inputs["golden"][".grm.bin"]) == NS * (NS + 1) // 2 * 4 == len(inputs["golden"][".grm.N.bin"])


@pytest.mark.parametrize("form,batch", [("plain", 1 << 16), ("plain", 1 << 22), ("bgzip", 1 << 16), ("bgzip", 1 << 22)])
def test_the_files_are_the_golden_writers(inputs, form, batch):
    prefix = str(inputs["tmp"] / ("out_%s_%d" % (form, batch)))
    n, ns = hpgv.run_grm(inputs["paths"][form], prefix, MIN_MAF, batch)
    assert (n, ns) == (inputs["n_used"], NS)
    got = _read(prefix)
    for sfx in SUFFIXES:
        assert got[sfx] == inputs["golden"][sfx], sfx


def test_refusals_write_no_file(inputs):
    prefix = str(inputs["tmp"] / "refused")
    vcf = inputs["paths"]["plain"]
    for v, p, m in ((None, prefix, 0.05), (vcf, None, 0.05), (vcf, prefix, 0.0), (vcf, prefix, -0.1), (vcf, prefix, 0.51), (vcf, prefix, float("nan"))):
        with pytest.raises(hpgv.HpgvError) as e:
            hpgv.run_grm(v, p, m)
        assert e.value.code == hpgv.ERR_INVALID
    with pytest.raises(hpgv.HpgvError):
        hpgv.run_grm(str(inputs["tmp"] / "missing.vcf"), prefix, 0.05)
    assert not any(os.path.exists(prefix + sfx) for sfx in SUFFIXES)


_RUNNER = """
import importlib, sys
sys.path.insert(0, %(root)r)
h = importlib.import_module("hpg-variant_amd")
print(*h.run_grm(sys.argv[1], sys.argv[2], float(sys.argv[3]), 1 << 16))
"""


def test_two_devices_write_the_same_files(inputs):
    """HPGV_DEVICES=0,0: two contexts on the one GPU, a buffer of sums each, added when the run ends"""
    script = inputs["tmp"] / "run.py"
    script.write_text(_RUNNER % {"root": ROOT})
    prefix = str(inputs["tmp"] / "two")
    env = dict(os.environ, HPGV_DEVICES="0,0")
    r = subprocess.run([sys.executable, str(script), inputs["paths"]["bgzip"], prefix, str(MIN_MAF)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(inputs["n_used"]), str(NS)]
    assert _read(prefix) == inputs["golden"]
