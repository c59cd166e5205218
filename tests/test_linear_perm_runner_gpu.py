"""hpgv_run_assoc_linear_perm: the linear regression's file runner with max(T) permutations.  Its result file is
hpgv_run_assoc_linear's byte for byte; the lines of <out>.mperm are the extended-precision oracle's empirical p-values under the
orders of the documented shuffle over the cohort that stayed; neither file depends on the batch size, the input form or the number
of engine threads; what is refused before anything is opened writes no file."""
import os
import subprocess
import sys

import numpy as np
import pytest

import linear_perm_golden as lp
from helpers import hpgv
from test_linear_runner_gpu import inputs, N_RECORDS, N_SAMPLES, _sorted          # noqa: F401  (the linear runner's files: 40 records x 60 samples, missing calls, 3 covariates)

pytestmark = pytest.mark.gpu

N_PERMS, SEED = 50, 2024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def expected(inputs):
    """the oracle's .mperm file, and the linear runner's result file"""
    used = inputs["has_trait"].copy()
    used[[inputs["absent"], inputs["cov_na"]]] = False
    cond = np.where(used, 0, 2).astype(np.uint8)                     # the trait's cohort: unaffected, everyone else OTHER
    order = lp.order_shuffle(cond, N_PERMS, SEED)
    coh = np.flatnonzero(used)
    idx = np.full(N_SAMPLES, -1)
    idx[coh] = np.arange(len(coh))
    cls = np.stack([r[3][coh] for r in inputs["rows"]])
    t_obs, T, ratio = lp.oracle(cls, inputs["trait"][coh], inputs["cov"][coh], idx[order[:, coh]])
    exp = dict(t_obs=t_obs, T=T, ratio=ratio, part=ratio > lp.EPS)
    c = lp.counts(exp, n_perms=N_PERMS)
    assert c["undecided"] == 0 and c["undecided_max"] == 0 and exp["part"].sum() == N_RECORDS - 1
    emp1, emp2 = hpgv.perm_pvalues(np.abs(t_obs), c["n_ge"], c["batch_max"])
    lines = ["#CHR\tPOS\tID\tEMP1\tEMP2\n"] + ["%s\t%d\t%s\t%s\t%s\n" % (ch, pos, vid, lp.format_f6(a), lp.format_f6(b))
                                                 for (ch, pos, vid, _), a, b in zip(inputs["rows"], emp1, emp2)]
    plain = str(inputs["tmp"] / "plain.linear")
    assert hpgv.run_assoc_linear(inputs["paths"]["plain"], inputs["ped"], None, inputs["covar"], plain) == (N_RECORDS, int(used.sum()))
    return dict(mperm=_sorted("".join(lines)), linear=open(plain, "rb").read(), used=int(used.sum()))


@pytest.mark.parametrize("form,batch", [("plain", 1 << 16), ("plain", 1 << 22), ("bgzip", 1 << 16), ("gzip", 1 << 20)])
def test_the_files_are_the_linear_runners_and_the_oracles(inputs, expected, form, batch):
    out = str(inputs["tmp"] / ("perm_%s_%d.linear" % (form, batch)))
    assert hpgv.run_assoc_linear_perm(inputs["paths"][form], inputs["ped"], None, inputs["covar"], out, N_PERMS, SEED, 0, batch) == (N_RECORDS, expected["used"])
    assert open(out, "rb").read() == expected["linear"]
    got = open(out + ".mperm", "rb").read()
    assert got.split(b"\n") == expected["mperm"].split(b"\n")
    assert got.count(b"\tnan\tnan\n") == 1                           # the monomorphic record takes no part


_RUNNER = """
import importlib, sys
sys.path.insert(0, %(root)r)
h = importlib.import_module("hpg-variant_amd")
print(*h.run_assoc_linear_perm(sys.argv[1], sys.argv[2], None, sys.argv[3], sys.argv[4], int(sys.argv[5]), int(sys.argv[6]), 0, 1 << 14))
"""


def test_another_number_of_engine_threads_writes_the_same_files(inputs, expected):
    script = inputs["tmp"] / "run_perm.py"
    script.write_text(_RUNNER % {"root": ROOT})
    out = str(inputs["tmp"] / "threads.linear")
    env = dict(os.environ, HPGV_ENGINE_THREADS="3")
    r = subprocess.run([sys.executable, str(script), inputs["paths"]["bgzip"], inputs["ped"], inputs["covar"], out, str(N_PERMS), str(SEED)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(N_RECORDS), str(expected["used"])]
    assert open(out, "rb").read() == expected["linear"] and open(out + ".mperm", "rb").read() == expected["mperm"]


def test_another_seed_and_the_plain_run_afterwards(inputs, expected):
    out = str(inputs["tmp"] / "seed.linear")
    assert hpgv.run_assoc_linear_perm(inputs["paths"]["plain"], inputs["ped"], None, inputs["covar"], out, N_PERMS, SEED + 1)[0] == N_RECORDS
    assert open(out, "rb").read() == expected["linear"] and open(out + ".mperm", "rb").read() != expected["mperm"]
    again = str(inputs["tmp"] / "after.linear")                      # the permutations end with their run
    assert hpgv.run_assoc_linear(inputs["paths"]["plain"], inputs["ped"], None, inputs["covar"], again)[0] == N_RECORDS
    assert open(again, "rb").read() == expected["linear"] and not os.path.exists(again + ".mperm")


def test_what_is_refused_before_anything_is_opened_writes_no_file(inputs):
    tmp, vcf, ped, covar = inputs["tmp"], inputs["paths"]["plain"], inputs["ped"], inputs["covar"]
    out = str(tmp / "refused_perm.linear")
    for args in [(vcf, ped, None, covar, out, 0, 1), (vcf, ped, None, covar, out, -3, 1), (None, ped, None, covar, out, 5, 1), (vcf, ped, None, covar, None, 5, 1),
                 (vcf, None, None, covar, out, 5, 1), (vcf, ped, None, None, out, 5, 1, 2), (vcf, ped, None, str(tmp / "missing.txt"), out, 5, 1)]:
        with pytest.raises(hpgv.HpgvError) as err:
            hpgv.run_assoc_linear_perm(*args)
        assert err.value.code == hpgv.ERR_INVALID, args
        assert not os.path.exists(out) and not os.path.exists(out + ".mperm"), args
