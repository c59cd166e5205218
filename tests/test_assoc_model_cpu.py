"""The model tests without a device: hpgv_run_assoc_model refuses bad arguments before the engine starts and writes nothing, and
the header's HPGV_MODEL_* values are the binding's."""
import os
import re

import pytest

from helpers import hpgv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bad_arguments_are_refused_before_the_engine_starts(tmp_path):
    vcf, ped, out = str(tmp_path / "in.vcf"), str(tmp_path / "ped.txt"), str(tmp_path / "out.model")
    open(vcf, "w").write("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS0\n1\t5\trs0\tA\tC\t.\tPASS\t.\tGT\t0/1\n")
    open(ped, "w").write("f S0 0 0 1 2\n")
    for args in ((vcf, ped, out, -1), (vcf, ped, out, -300), (None, ped, out, 0), (vcf, None, out, 5), (vcf, ped, None, 5)):
        with pytest.raises(hpgv.HpgvError) as err:
            hpgv.run_assoc_model(args[0], args[1], args[2], n_perms=args[3], seed=1)
        assert err.value.code == hpgv.ERR_INVALID
    assert not os.path.exists(out) and not os.path.exists(out + ".mperm")


def test_model_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "hpgv.h")).read()
    values = {k: int(v) for k, v in re.findall(r"HPGV_MODEL_(\w+) = (\d+)", text)}
    assert values == dict(GENO=hpgv.MODEL_GENO, TREND=hpgv.MODEL_TREND, ALLELIC=hpgv.MODEL_ALLELIC, DOM=hpgv.MODEL_DOM, REC=hpgv.MODEL_REC)
    assert [values[k] for k in ("GENO", "TREND", "ALLELIC", "DOM", "REC")] == [0, 1, 2, 3, 4]
    for name in ("hpgv_assoc_model_scan_dev", "hpgv_assoc_model_stats_dev", "hpgv_assoc_trend_perm_dev", "hpgv_assoc_model", "hpgv_assoc_model_text"):
        assert name in hpgv.SYMBOLS and hasattr(hpgv.load(), name)
