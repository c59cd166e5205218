"""hpgv_run_set_record_filters (--region, --region-file / --region-type, --coverage, --snp, --var-type, --indel, --inh-dom,
--inh-rec; shared_options.c:42-56,86-173): the refusals.  A bad setting is refused when it is set and leaves the previous
one in force; an inheritance filter without a PED is refused before the engine starts.  No GPU: a call that got as far
as the engine would fail for want of a device, so a clean HPGV_ERR_INVALID with no engine bound and no file written shows
the checks come first."""
import ctypes as C
import os
from importlib import import_module

import pytest

from helpers import hpgv

HPGV_ERR_INVALID = 1


class _Filters(C.Structure):
    _fields_ = [("min_maf", C.c_double), ("max_missing", C.c_double), ("max_mendel_errors", C.c_int),
                ("num_alleles", C.c_int), ("min_quality", C.c_double)]


class _RecFilters(C.Structure):
    _fields_ = [("min_coverage", C.c_long), ("regions", C.c_char_p), ("region_file", C.c_char_p), ("region_type", C.c_char_p),
                ("snp", C.c_int), ("var_type", C.c_int), ("indel", C.c_int), ("min_dominant", C.c_double), ("min_recessive", C.c_double)]


def rec(**kw):
    f = _RecFilters(-1, None, None, None, -1, -1, -1, -1.0, -1.0)
    for k, v in kw.items():
        setattr(f, k, v.encode() if isinstance(v, str) else v)
    return f


@pytest.fixture(scope="module")
def host():
    hpgv.build()
    L = C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)
    L.hpgv_run_filter.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.hpgv_run_assoc.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long)]
    L.hpgv_run_aggregate.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long)]
    L.hpgv_run_set_filters.argtypes = [C.POINTER(_Filters)]
    L.hpgv_run_set_record_filters.argtypes = [C.POINTER(_RecFilters)]
    L.hpgv_host_last_error.restype = C.c_char_p
    L.hpgv_run_set_filters(None)
    L.hpgv_host_shutdown()                                     # no engine bound by an earlier test of the same process
    yield L
    L.hpgv_run_set_record_filters(None)


@pytest.fixture
def tmp(tmp_path, host):
    (tmp_path / "in.vcf").write_text("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\n"
                                     "1\t10\trs1\tA\tC\t50\tPASS\tDP=4\tGT\t0/1\n")
    yield tmp_path
    host.hpgv_run_set_record_filters(None)
    assert sorted(os.listdir(tmp_path)) == sorted(["in.vcf"] + [f for f in os.listdir(tmp_path) if f.endswith(".gff")])
    assert host.hpgv_host_device_count() == 0                  # the engine was never bound


def _filter_without_ped(host, tmp):
    rc = host.hpgv_run_filter(str(tmp / "in.vcf").encode(), None, str(tmp / "out").encode(), 1, 1 << 16, None, None)
    return rc, host.hpgv_host_last_error()


def _refused_keeping(host, tmp, bad):
    """`bad` is refused; an inheritance setting made before stays in force, and so does 'all off'"""
    assert host.hpgv_run_set_record_filters(C.byref(rec(min_dominant=0.5))) == 0
    assert host.hpgv_run_set_record_filters(C.byref(bad)) == HPGV_ERR_INVALID
    assert host.hpgv_host_last_error()
    rc, msg = _filter_without_ped(host, tmp)                   # the inheritance filter still there: it needs a PED
    assert rc == HPGV_ERR_INVALID and b"PED" in msg and b"inheritance" in msg, msg
    assert host.hpgv_run_set_record_filters(None) == 0
    assert host.hpgv_run_set_record_filters(C.byref(bad)) == HPGV_ERR_INVALID
    rc, msg = _filter_without_ped(host, tmp)                   # still none: the filter tool refuses to run without one
    assert rc == HPGV_ERR_INVALID and b"no filter" in msg, msg


@pytest.mark.parametrize("regions", ["1:200-100", "1:a-5", ":5", "1,,2", "", "1:", "1:5-", "1:0-4", "2,"])
def test_malformed_regions_are_refused(host, tmp, regions):
    _refused_keeping(host, tmp, rec(regions=regions))


def test_missing_region_file_is_refused(host, tmp):
    _refused_keeping(host, tmp, rec(region_file=str(tmp / "absent.gff")))


@pytest.mark.parametrize("row", ["1\tsrc\tgene\t100", "1\tsrc\tgene\tx100\t200\t.\t+\t.\tID=a", "1\tsrc\tgene\t300\t200\t.\t+\t.\tID=a",
                                 "\tsrc\tgene\t1\t2\t.\t+\t.\tID=a"])
def test_malformed_gff_rows_are_refused(host, tmp, row):
    gff = tmp / "bad.gff"
    gff.write_text("##gff-version 3\n1\tsrc\texon\t5\t10\t.\t+\t.\tID=e\n\n" + row + "\n")
    _refused_keeping(host, tmp, rec(region_file=str(gff), region_type="exon"))     # every row is checked, whatever its feature


@pytest.mark.parametrize("bad", [dict(min_dominant=1.5), dict(min_recessive=1.5), dict(min_dominant=float("nan")), dict(var_type=7),
                                 dict(var_type=0), dict(snp=2), dict(indel=-2), dict(region_type="gene")])
def test_out_of_range_values_are_refused(host, tmp, bad):
    _refused_keeping(host, tmp, rec(**bad))


def test_well_formed_settings_are_taken(host, tmp):
    gff = tmp / "ok.gff"
    gff.write_text("##gff-version 3\n# a comment\n\n1\tsrc\tgene\t100\t200\t.\t+\t.\tID=g\r\nchr2\tsrc\texon\t5\t5\n")
    for f in (rec(regions="1"), rec(regions="chr1:5,1:100-200,HLA:A:7-9"), rec(region_file=str(gff)),
              rec(region_file=str(gff), region_type="exon"), rec(min_coverage=0, snp=0, var_type=3, indel=1),
              rec(min_dominant=1.0, min_recessive=0.0)):
        assert host.hpgv_run_set_record_filters(C.byref(f)) == 0, host.hpgv_host_last_error()
    assert host.hpgv_run_set_record_filters(C.byref(rec())) == 0    # nothing active: the same as all off
    rc, msg = _filter_without_ped(host, tmp)
    assert rc == HPGV_ERR_INVALID and b"no filter" in msg


def test_inheritance_without_ped_is_refused_by_every_runner(host, tmp):
    vcf, out = str(tmp / "in.vcf").encode(), str(tmp / "out").encode()
    assert host.hpgv_run_set_record_filters(C.byref(rec(min_dominant=0.9))) == 0
    assert host.hpgv_run_filter(vcf, None, out, 0, 1 << 16, None, None) == HPGV_ERR_INVALID
    assert b"PED" in host.hpgv_host_last_error()
    n = C.c_long(-7)
    assert host.hpgv_run_assoc(vcf, None, out, 1, 1 << 16, C.byref(n)) == HPGV_ERR_INVALID
    assert b"PED" in host.hpgv_host_last_error()
    assert host.hpgv_run_set_record_filters(C.byref(rec(min_recessive=0.2, regions="1:1-20"))) == 0
    assert host.hpgv_run_aggregate(vcf, out, 0, 1 << 16, C.byref(n)) == HPGV_ERR_INVALID       # aggregate takes no PED
    assert b"inheritance" in host.hpgv_host_last_error()
