"""hpgv_run_filter (hpg-var-vcf filter, filter_runner.c:23-260): the refusals that come before the engine starts.  No GPU:
a call that got as far as the engine would fail here for want of a device, so a clean HPGV_ERR_INVALID with no engine
bound and no file written shows the checks come first."""
import ctypes as C
import os
from importlib import import_module

import pytest

from helpers import hpgv

HPGV_ERR_INVALID = 1


class _Filters(C.Structure):
    _fields_ = [("min_maf", C.c_double), ("max_missing", C.c_double), ("max_mendel_errors", C.c_int),
                ("num_alleles", C.c_int), ("min_quality", C.c_double)]


@pytest.fixture(scope="module")
def host():
    hpgv.build()
    L = C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)
    L.hpgv_run_filter.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.hpgv_run_set_filters.argtypes = [C.POINTER(_Filters)]
    L.hpgv_host_last_error.restype = C.c_char_p
    yield L
    L.hpgv_run_set_filters(None)


def _vcf(tmp_path):
    p = tmp_path / "in.vcf"
    p.write_text("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\n1\t10\trs1\tA\tC\t50\tPASS\t.\tGT\t0/1\n")
    return str(p).encode()


def test_status_code_is_the_headers():
    assert hpgv.ERR_INVALID == HPGV_ERR_INVALID


def test_no_filter_writes_nothing_and_starts_no_engine(host, tmp_path):
    host.hpgv_run_set_filters(None)
    npass, nrej = C.c_long(7), C.c_long(7)
    rc = host.hpgv_run_filter(_vcf(tmp_path), None, str(tmp_path / "out").encode(), 1, 1 << 16, C.byref(npass), C.byref(nrej))
    assert rc == HPGV_ERR_INVALID
    assert b"no filter" in host.hpgv_host_last_error()
    assert npass.value == 0 and nrej.value == 0
    assert sorted(os.listdir(tmp_path)) == ["in.vcf"]
    assert host.hpgv_host_device_count() == 0                  # the engine was never bound


def test_null_paths_and_mendel_without_ped_are_refused(host, tmp_path):
    host.hpgv_run_set_filters(C.byref(_Filters(-1, -1, -1, -1, 30.0)))
    try:
        out = str(tmp_path / "out").encode()
        assert host.hpgv_run_filter(None, None, out, 0, 1 << 16, None, None) == HPGV_ERR_INVALID
        assert host.hpgv_run_filter(_vcf(tmp_path), None, None, 0, 1 << 16, None, None) == HPGV_ERR_INVALID
        host.hpgv_run_set_filters(C.byref(_Filters(-1, -1, 0, -1, -1)))
        assert host.hpgv_run_filter(_vcf(tmp_path), None, out, 0, 1 << 16, None, None) == HPGV_ERR_INVALID
        assert b"PED" in host.hpgv_host_last_error()
    finally:
        host.hpgv_run_set_filters(None)
    assert sorted(os.listdir(tmp_path)) == ["in.vcf"]
    assert host.hpgv_host_device_count() == 0
