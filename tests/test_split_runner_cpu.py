"""hpgv_run_split (hpg-var-vcf split, split_runner.c:23-190): the refusals that come before the engine starts.  No GPU: a
call that got as far as the engine would fail here for want of a device, so a clean HPGV_ERR_INVALID with no engine bound and
no file written shows the checks come first."""
import ctypes as C
import os
from importlib import import_module

import pytest

from helpers import hpgv

HPGV_ERR_INVALID = 1
CHROMOSOME, COVERAGE = 1, 2


@pytest.fixture(scope="module")
def host():
    hpgv.build()
    L = C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)
    L.hpgv_run_split.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_long), C.c_int, C.c_size_t,
                                 C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.hpgv_host_last_error.restype = C.c_char_p
    L.hpgv_host_shutdown()                                     # no engine bound by an earlier test of the same process
    return L


def _vcf(tmp_path):
    p = tmp_path / "in.vcf"
    p.write_text("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\n1\t10\trs1\tA\tC\t50\tPASS\tDP=3\tGT\t0/1\n")
    return str(p).encode()


def _split(host, vcf, out, criterion, intervals):
    iv = (C.c_long * max(1, len(intervals or [])))(*(intervals or []))
    counts = [C.c_long(7), C.c_long(7), C.c_long(7)]
    rc = host.hpgv_run_split(vcf, out, criterion, iv if intervals is not None else None, len(intervals or []), 1 << 16,
                             *[C.byref(c) for c in counts])
    assert [c.value for c in counts] == [0, 0, 0]
    return rc


@pytest.mark.parametrize("case", ["null_vcf", "null_dir", "criterion_0", "criterion_3", "coverage_no_intervals",
                                  "coverage_null_intervals", "coverage_equal", "coverage_decreasing"])
def test_refusals_write_nothing_and_start_no_engine(host, tmp_path, case):
    vcf, out = _vcf(tmp_path), str(tmp_path / "out").encode()
    args = {"null_vcf": (None, out, CHROMOSOME, None), "null_dir": (vcf, None, CHROMOSOME, None),
            "criterion_0": (vcf, out, 0, None), "criterion_3": (vcf, out, 3, [10]),
            "coverage_no_intervals": (vcf, out, COVERAGE, []), "coverage_null_intervals": (vcf, out, COVERAGE, None),
            "coverage_equal": (vcf, out, COVERAGE, [5, 10, 10, 20]), "coverage_decreasing": (vcf, out, COVERAGE, [30, 20])}[case]
    assert _split(host, *args) == HPGV_ERR_INVALID
    assert host.hpgv_host_last_error()
    assert sorted(os.listdir(tmp_path)) == ["in.vcf"]          # not even the output directory
    assert host.hpgv_host_device_count() == 0                  # the engine was never bound


def test_an_out_dir_that_cannot_be_created_is_refused(host, tmp_path):
    vcf = _vcf(tmp_path)
    (tmp_path / "file").write_text("x")
    for out in (tmp_path / "missing" / "two_levels", tmp_path / "file"):
        assert _split(host, vcf, str(out).encode(), CHROMOSOME, None) == HPGV_ERR_INVALID
        assert b"output directory" in host.hpgv_host_last_error()
    assert sorted(os.listdir(tmp_path)) == ["file", "in.vcf"]
    assert host.hpgv_host_device_count() == 0
