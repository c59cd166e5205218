"""hpgv_run_assoc_clump: the association run that also writes <out>.clumped.  The result file is hpgv_run_assoc's, byte for byte;
the clumps are what a Python path gives -- the engine's own p-values over the whole file in one call (Engine.assoc_text), numpy r2
between the candidate rows (ld_golden.band) and the direct clump loop (clump_golden.clump_loop) -- whatever the batch size and the
input form."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import clump_golden as cg
import ld_golden as lg
from helpers import hpgv
from oracle import pyoracle as orc
from test_host_logic_cpu import _bgzf

pytestmark = pytest.mark.gpu

N_AFF, N_UNAFF, N_BLOCKS, BLOCK = 60, 60, 30, 10
N_VARIANTS = N_BLOCKS * BLOCK
MIN_R2 = 0.5


@pytest.fixture(scope="module")
def host():
    hpgv.build()
    from importlib import import_module
    b = import_module("hpg-variant_amd._build")
    L = C.CDLL(b.HOSTLIB)
    L.hpgv_run_assoc.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long)]
    yield L
    L.hpgv_host_shutdown()


def _genotypes():
    """300 rows x 120 samples (affected first): 30 blocks of 10 -- a founder row, in every third block with the affected allele
    frequency raised by 0.25, and nine rows that are the founder with 0 %, 3 %, 10 % or 30 % of its genotypes redrawn.  Blocks are
    interleaved in pairs, so the members of a block are not adjacent rows.  3 = missing"""
    rng = np.random.default_rng(4242)
    ns = N_AFF + N_UNAFF
    rows = np.zeros((N_VARIANTS, ns), np.int64)
    for blk in range(N_BLOCKS):
        freq = np.full(ns, 0.3)
        if blk % 3 == 0:
            freq[:N_AFF] += 0.25
        founder = rng.binomial(2, freq)
        pair, odd = divmod(blk, 2)
        for k in range(BLOCK):
            share = (0.0, 0.0, 0.03, 0.10, 0.30)[0 if k == 0 else 1 + (k - 1) % 4]
            redraw = rng.random(ns) < share
            g = np.where(redraw, rng.binomial(2, 0.3, ns), founder)
            g = np.where(rng.random(ns) < 0.01, 3, g)
            rows[pair * 2 * BLOCK + 2 * k + odd] = g
    return rows


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("clump_runner")
    g = _genotypes()
    ns = g.shape[1]
    rng = np.random.default_rng(5)
    cols = rng.permutation(ns)                                      # VCF column j holds sample cols[j]
    names = ["S%d" % s for s in cols]
    with open(tmp / "ped.txt", "w") as f:
        for s in range(ns):
            f.write("fam%d S%d 0 0 %d %d\n" % (s, s, 1 + s % 2, 2 if s < N_AFF else 1))
    cond = np.array([orc.AFFECTED if s < N_AFF else orc.UNAFFECTED for s in cols], np.uint8)
    gt_text = np.array(["0/0", "0/1", "1/1", "./."])
    head = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n"
    out = dict(tmp=tmp, ped=str(tmp / "ped.txt"), cond=cond)
    # one chromosome; two chromosomes, the change inside a pair of blocks (rows 140 .. 159)
    for name, chrom_of in (("one", lambda v: "1"), ("two", lambda v: "1" if v < 150 else "2")):
        chrom = [chrom_of(v) for v in range(N_VARIANTS)]
        pos = [1000 + 10 * v for v in range(N_VARIANTS)]
        body = "".join("%s\t%d\trs%d\tA\tC\t.\tPASS\t.\tGT\t%s\n" % (chrom[v], pos[v], v, "\t".join(gt_text[g[v, cols]])) for v in range(N_VARIANTS))
        data = (head + body).encode()
        plain, bgz = str(tmp / (name + ".vcf")), str(tmp / (name + "_bgz.vcf.gz"))
        open(plain, "wb").write(data)
        open(bgz, "wb").write(_bgzf(data, 0x4000))
        assert len(data) > 2 * (1 << 16)                           # batches hold at most 64 KiB of whole lines: those runs are at least three
        e = hpgv.Engine(0)
        e.set_cohort(cond)
        res = e.assoc_text(hpgv.TASK_CHISQ, body.encode())
        e.close()
        assert res["n_lines"] == N_VARIANTS and not res["status"].any()
        codes = orc.tokenize(body, ns, True)["gt"]
        out[name] = dict(plain=plain, bgzip=bgz, chrom=chrom, pos=np.array(pos), p=res["p"].copy(), codes=codes)
    return out


def _midpoint(p, near):
    """a threshold next to `near` that no p lies close to: the midpoint of the two sorted p-values around it"""
    ps = np.sort(p[~np.isnan(p)])
    k = int(np.searchsorted(ps, near))
    assert 0 < k < len(ps) and ps[k - 1] < ps[k]
    return 0.5 * (ps[k - 1] + ps[k])


def _expected(case, p1, p2, window, max_bp):
    """(the clumps as (ID, P, TOTAL, SP2) in clump order, the number of truncated candidates, facts about the reference)"""
    p, chrom, pos = case["p"], case["chrom"], case["pos"]
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(p <= p2)
    n = len(cand)
    names = {}
    ch = np.array([names.setdefault(chrom[v], len(names)) for v in cand], np.int32)
    r2 = lg.band(case["codes"][cand], window, chrom=ch, pos=pos[cand], max_bp=max_bp)[0]
    edges = cg.edges_of_band(r2, MIN_R2)
    pairs = list(zip(edges["a"].tolist(), edges["b"].tolist()))
    index_of, order = cg.clump_loop(p[cand].tolist(), pairs, p1)
    clumps = []
    for i in order:
        members = [j for j in range(n) if index_of[j] == i and j != i]
        sp2 = ",".join("%s:%d" % (chrom[cand[j]], pos[cand[j]]) for j in members) or "NONE"
        clumps.append(("rs%d" % cand[i], float(p[cand[i]]), len(members), sp2, chrom[cand[i]], int(pos[cand[i]])))
    trunc = sum(1 for i in range(n - window - 1)
                if ch[i + window + 1] == ch[i] and (max_bp < 0 or abs(int(pos[cand[i + window + 1]]) - int(pos[cand[i]])) <= max_bp))
    facts = dict(candidates=n, clumps=len(order), sizes=[c[2] for c in clumps],
                 claimed_hits=int(sum(1 for j in range(n) if p[cand[j]] <= p1 and index_of[j] not in (-1, j))),
                 unclaimed=int((index_of == -1).sum()))
    return clumps, trunc, facts


def _check_clumped(path, clumps):
    lines = open(path).read().split("\n")
    assert lines[0] == "#CHR\tPOS\tID\tP\tTOTAL\tSP2" and lines[-1] == ""
    body = lines[1:-1]
    assert len(body) == len(clumps)
    for line, (rid, p, total, sp2, chrom, pos) in zip(body, clumps):
        f = line.split("\t")
        assert len(f) == 6
        assert (f[0], int(f[1]), f[2]) == (chrom, pos, rid)
        assert f[3] == "%.6e" % float(f[3]) and abs(float(f[3]) - p) <= 1e-6 * p
        assert int(f[4]) == total and f[5] == sp2


def test_the_reference_has_every_kind_of_clump(inputs):
    case = inputs["one"]
    p1, p2 = _midpoint(case["p"], 1e-3), _midpoint(case["p"], 1e-2)
    clumps, trunc, facts = _expected(case, p1, p2, 1024, 250000)
    print(facts)
    assert facts["clumps"] >= 3 and max(facts["sizes"]) >= 2 and min(facts["sizes"]) == 0
    assert facts["claimed_hits"] >= 1 and facts["unclaimed"] >= 1 and trunc == 0


@pytest.mark.parametrize("form,batch,window,max_bp,which", [
    ("plain", 1 << 22, 1024, 250000, "one"),
    ("plain", 1 << 16, 1024, 250000, "one"),                        # at least three batches
    ("bgzip", 1 << 16, 1024, 250000, "one"),
    ("plain", 1 << 16, 4, 250000, "one"),                           # the candidate window cuts the distance window short
    ("plain", 1 << 22, 1024, -1, "one"),
    ("plain", 1 << 16, 1024, 60, "two"),                            # two chromosomes, and a distance limit that cuts every block
    ("bgzip", 1 << 22, 1024, 250000, "two"),
])
def test_clumped_file(host, inputs, form, batch, window, max_bp, which):
    case = inputs[which]
    p1, p2 = _midpoint(case["p"], 1e-3), _midpoint(case["p"], 1e-2)
    clumps, trunc, facts = _expected(case, p1, p2, window, max_bp)
    tag = "%s_%s_%d_%d_%d" % (which, form, batch, window, max_bp)
    out, plain_out = str(inputs["tmp"] / (tag + ".chisq")), str(inputs["tmp"] / (tag + ".assoc"))
    n, n_clumps, n_trunc = hpgv.run_assoc_clump(case[form], inputs["ped"], out, hpgv.TASK_CHISQ, p1=p1, p2=p2, min_r2=MIN_R2, max_bp=max_bp,
                                                window=window, batch_bytes=batch)
    assert n == N_VARIANTS and n_clumps == len(clumps) and n_trunc == trunc
    if window == 4:
        assert trunc > 0
    if max_bp == 60:
        one = _expected(case, p1, p2, window, 250000)[0]
        assert [c[3] for c in clumps] != [c[3] for c in one], "the distance limit cut no clump"
    _check_clumped(out + ".clumped", clumps)
    k = C.c_long(0)
    assert host.hpgv_run_assoc(case[form].encode(), inputs["ped"].encode(), plain_out.encode(), 1, batch, C.byref(k)) == 0 and k.value == n
    assert open(out, "rb").read() == open(plain_out, "rb").read()


_CHILD = """
import sys
from importlib import import_module
sys.path.insert(0, %(root)r)
hpgv = import_module("hpg-variant_amd")
vcf, ped, out, p1, p2 = sys.argv[1:6]
print(*hpgv.run_assoc_clump(vcf, ped, out, p1=float(p1), p2=float(p2), min_r2=0.5, batch_bytes=1 << 16))
"""


def test_devices_and_kernel_chains_write_the_same_files(inputs):
    """a group of two contexts (HPGV_DEVICES=0,0: four engine threads, the edges on member 0) and the kernel chains
    (HPGV_BATCH_FUSED=0) in processes of their own, against this process's run"""
    case, tmp = inputs["one"], inputs["tmp"]
    p1, p2 = _midpoint(case["p"], 1e-3), _midpoint(case["p"], 1e-2)
    here = str(tmp / "here.out")
    counts = hpgv.run_assoc_clump(case["plain"], inputs["ped"], here, p1=p1, p2=p2, min_r2=MIN_R2, batch_bytes=1 << 16)
    assert counts[1] >= 3
    script = tmp / "child.py"
    script.write_text(_CHILD % {"root": os.path.dirname(os.path.dirname(os.path.abspath(__file__)))})
    for tag, extra in (("group", {"HPGV_DEVICES": "0,0"}), ("chains", {"HPGV_BATCH_FUSED": "0"})):
        env = {k: v for k, v in os.environ.items() if k not in ("HPGV_DEVICES", "HPGV_BATCH_FUSED")}
        env.update(extra)
        out = str(tmp / (tag + ".out"))
        r = subprocess.run([sys.executable, str(script), case["plain"], inputs["ped"], out, repr(float(p1)), repr(float(p2))], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert tuple(int(x) for x in r.stdout.split()) == counts
        assert open(out, "rb").read() == open(here, "rb").read()
        assert open(out + ".clumped", "rb").read() == open(here + ".clumped", "rb").read()


def test_fisher_task_and_no_candidate(host, inputs):
    case = inputs["one"]
    out = str(inputs["tmp"] / "fisher.out")
    n, n_clumps, n_trunc = hpgv.run_assoc_clump(case["plain"], inputs["ped"], out, hpgv.TASK_FISHER, p1=1e-3, p2=1e-2)
    assert n == N_VARIANTS and n_clumps >= 3
    lines = open(out + ".clumped").read().split("\n")
    assert len(lines) == n_clumps + 2
    # thresholds below every p: the header alone
    out = str(inputs["tmp"] / "none.out")
    assert hpgv.run_assoc_clump(case["plain"], inputs["ped"], out, p1=1e-300, p2=1e-300) == (N_VARIANTS, 0, 0)
    assert open(out + ".clumped").read() == "#CHR\tPOS\tID\tP\tTOTAL\tSP2\n"


def test_refusals(inputs):
    case, tmp = inputs["one"], inputs["tmp"]
    out = str(tmp / "refused.out")
    nan = float("nan")
    bad = [dict(p1=0.0), dict(p2=0.0), dict(p1=1.5, p2=1.5), dict(p2=1.5), dict(p1=-1e-3), dict(p1=1e-2, p2=1e-3), dict(p1=nan), dict(p2=nan),
           dict(min_r2=nan), dict(window=0), dict(window=1025), dict(window=-1)]
    for kw in bad:
        with pytest.raises(hpgv.HpgvError) as err:
            hpgv.run_assoc_clump(case["plain"], inputs["ped"], out, **kw)
        assert err.value.code == hpgv.ERR_INVALID, kw
    for vcf, ped, o, opt in ((None, inputs["ped"], out, None), (case["plain"], None, out, None), (case["plain"], inputs["ped"], None, None),
                             (case["plain"], inputs["ped"], out, False)):
        with pytest.raises(hpgv.HpgvError) as err:
            hpgv.run_assoc_clump(vcf, ped, o, options=opt)
        assert err.value.code == hpgv.ERR_INVALID
    with pytest.raises(hpgv.HpgvError) as err:
        hpgv.run_assoc_clump(case["plain"], inputs["ped"], out, task=7)
    assert err.value.code == hpgv.ERR_INVALID
    assert not os.path.exists(out) and not os.path.exists(out + ".clumped")
    # p1 == p2 == 1 is legal
    ok = str(tmp / "all.out")
    n, n_clumps, _ = hpgv.run_assoc_clump(case["plain"], inputs["ped"], ok, p1=1.0, p2=1.0)
    assert n == N_VARIANTS and n_clumps > 0
