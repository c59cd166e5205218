"""hpgv_run_filter and hpgv_run_split with hpgv_run_set_output_compression(HPGV_OUT_BGZF): the files are bgzip -- whole BGZF
members and one EOF block at the end -- and inflate, byte for byte, to what the same run writes as plain text; from plain,
gzip and bgzip input, from the default batch size, from dozens of batches and with a one-line last batch; split files that
were closed and opened again keep one EOF block; the tools read their own output."""
import ctypes as C
import gzip
import os
import struct
from importlib import import_module

import numpy as np
import pytest

from helpers import hpgv
from test_host_logic_cpu import _bgzf

pytestmark = pytest.mark.gpu

OUT_PLAIN, OUT_BGZF = 0, 1
EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
SPLIT_CHROMOSOME, SPLIT_COVERAGE = 1, 2


class _Filters(C.Structure):
    _fields_ = [("min_maf", C.c_double), ("max_missing", C.c_double), ("max_mendel_errors", C.c_int),
                ("num_alleles", C.c_int), ("min_quality", C.c_double)]


@pytest.fixture(scope="module")
def host():
    hpgv.build()
    L = C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)
    L.hpgv_run_filter.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.hpgv_run_split.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_long), C.c_int, C.c_size_t,
                                 C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.hpgv_run_set_filters.argtypes = [C.POINTER(_Filters)]
    L.hpgv_host_last_error.restype = C.c_char_p
    text = open(os.path.join(import_module("hpg-variant_amd._build").ROOT, "include", "hpgv_host.h")).read()
    assert "HPGV_SPLIT_CHROMOSOME = 1, HPGV_SPLIT_COVERAGE = 2" in text
    yield L
    L.hpgv_run_set_output_compression(OUT_PLAIN)
    L.hpgv_run_set_filters(None)
    L.hpgv_host_shutdown()


def _records(n_records, n_samples, n_contigs, seed):
    rng = np.random.default_rng(seed)
    names = ["s%d" % k for k in range(n_samples)]
    hdr = ("##fileformat=VCFv4.1\n##source=test\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n").encode()
    lines = []
    for v in range(n_records):
        af = rng.random() * 0.5
        a = rng.random((n_samples, 2)) < af
        sep = np.where(rng.random(n_samples) < 0.5, "/", "|")
        miss = rng.random(n_samples) < 0.02
        gts = "\t".join("./." if m else "%d%s%d" % (x, s, y) for (x, y), s, m in zip(a, sep, miss))
        chrom = "ctg%d" % (v * n_contigs // n_records if v % 3 else int(rng.integers(0, n_contigs)))      # runs, and strays that reopen files
        info = "DP=%d" % int(rng.integers(0, 120)) if v % 11 else "NS=3"
        lines.append(("%s\t%d\trs%d\tA\tC\t%d\tPASS\t%s\tGT\t%s\n" % (chrom, 1000 + v, v, int(rng.integers(0, 60)), info, gts)).encode())
    return hdr, lines


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    """1 500 records of 100 samples (~650 KB): dozens of 64 KiB batches; the last record alone is shorter than the room a 64 KiB
    batch leaves only by construction of `one_line_batch` below"""
    tmp = tmp_path_factory.mktemp("bgzf_out")
    hdr, lines = _records(1500, 100, 80, 5)
    data = hdr + b"".join(lines)
    paths = {"plain": tmp / "in.vcf", "gzip": tmp / "in.vcf.gzip.gz", "bgzip": tmp / "in.vcf.gz"}
    paths["plain"].write_bytes(data)
    paths["gzip"].write_bytes(gzip.compress(data, 6))
    paths["bgzip"].write_bytes(_bgzf(data, 0x4000))
    # a batch size that leaves the last line a batch of its own: everything but the last line fits exactly
    one_line_batch = len(b"".join(lines[:-1]))
    return dict(tmp=tmp, paths={k: str(v) for k, v in paths.items()}, one_line_batch=one_line_batch, n=len(lines))


def _walk(data):
    """a bgzip file: whole members of at most 65 536 bytes by BSIZE, the last one the EOF block, no other EOF block"""
    at, members = 0, []
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00", at
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert size <= 65536 and at + size <= len(data)
        assert struct.unpack_from("<I", data, at + size - 4)[0] <= 65280
        members.append(data[at:at + size])
        at += size
    assert members and members[-1] == EOF and EOF not in members[:-1]
    return members


def _filter(host, vcf, prefix, save, batch, mode):
    F = _Filters(-1, -1, -1, -1, 30.0)
    host.hpgv_run_set_filters(C.byref(F))
    if mode is not None:
        assert host.hpgv_run_set_output_compression(mode) == 0
    npass, nrej = C.c_long(-1), C.c_long(-1)
    try:
        rc = host.hpgv_run_filter(vcf.encode(), None, prefix.encode(), save, batch, C.byref(npass), C.byref(nrej))
    finally:
        host.hpgv_run_set_filters(None)
    assert rc == 0, host.hpgv_host_last_error()
    return npass.value, nrej.value


def test_default_mode_writes_plain_names(host, cohort):
    # first in the module: the setter has not been called in this process
    prefix = str(cohort["tmp"] / "default")
    _filter(host, cohort["paths"]["plain"], prefix, 1, 1 << 22, None)
    assert os.path.exists(prefix + ".filtered") and os.path.exists(prefix + ".rejected")
    assert not os.path.exists(prefix + ".filtered.gz") and not os.path.exists(prefix + ".rejected.gz")
    assert open(prefix + ".filtered", "rb").read().startswith(b"##fileformat")


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzip"])
@pytest.mark.parametrize("save", [0, 1])
def test_filter_inflates_to_the_plain_run(host, cohort, kind, save):
    for batch in (1 << 22, 1 << 16, cohort["one_line_batch"]):
        tag = "%s_%d_%d" % (kind, save, batch)
        p_plain, p_gz = str(cohort["tmp"] / ("p_" + tag)), str(cohort["tmp"] / ("z_" + tag))
        counts = _filter(host, cohort["paths"][kind], p_plain, save, batch, OUT_PLAIN)
        assert _filter(host, cohort["paths"][kind], p_gz, save, batch, OUT_BGZF) == counts
        assert 0 < counts[0] < cohort["n"]
        assert not os.path.exists(p_gz + ".filtered") and not os.path.exists(p_gz + ".rejected")
        for ext in (".filtered", ".rejected"):
            packed = open(p_gz + ext + ".gz", "rb").read()
            _walk(packed)
            assert packed.endswith(EOF)
            assert gzip.decompress(packed) == open(p_plain + ext, "rb").read(), (tag, ext)
        if not save:
            assert open(p_gz + ".rejected.gz", "rb").read() == EOF          # a valid, empty bgzip file
    host.hpgv_run_set_output_compression(OUT_PLAIN)


def test_last_line_without_newline_and_empty_lines(host, tmp_path):
    hdr, lines = _records(400, 20, 3, 9)
    lines[0] = b"\n"; lines[20] = b"\n"; lines[21] = b"\n"; lines[10] = b"ctg0\t110\n"
    for last_q in (45, 5):                                       # the unterminated last line kept, then rejected
        data = hdr + b"".join(lines) + b"ctg1\t999999\trs_last\tA\tC\t%d\tPASS\t.\tGT\t" % last_q + b"\t".join([b"0/1"] * 20)
        for kind in ("plain", "bgzip"):
            vcf = tmp_path / ("in_%s_%d.vcf" % (kind, last_q))
            vcf.write_bytes(data if kind == "plain" else _bgzf(data, 0x1000))
            a, b = str(tmp_path / ("a%s%d" % (kind, last_q))), str(tmp_path / ("b%s%d" % (kind, last_q)))
            assert _filter(host, str(vcf), a, 1, 1 << 16, OUT_PLAIN) == _filter(host, str(vcf), b, 1, 1 << 16, OUT_BGZF)
            for ext in (".filtered", ".rejected"):
                packed = open(b + ext + ".gz", "rb").read()
                _walk(packed)
                assert gzip.decompress(packed) == open(a + ext, "rb").read(), (kind, last_q, ext)
    host.hpgv_run_set_output_compression(OUT_PLAIN)


def _split(host, vcf, out_dir, criterion, batch, mode):
    assert host.hpgv_run_set_output_compression(mode) == 0
    iv = (C.c_long * 3)(20, 50, 90)
    nrec, nfiles, nskip = C.c_long(-1), C.c_long(-1), C.c_long(-1)
    rc = host.hpgv_run_split(vcf.encode(), out_dir.encode(), criterion, iv if criterion == SPLIT_COVERAGE else None,
                             3 if criterion == SPLIT_COVERAGE else 0, batch, C.byref(nrec), C.byref(nfiles), C.byref(nskip))
    assert rc == 0, host.hpgv_host_last_error()
    return nrec.value, nfiles.value, nskip.value


@pytest.mark.parametrize("criterion", [SPLIT_CHROMOSOME, SPLIT_COVERAGE])
@pytest.mark.parametrize("kind", ["plain", "bgzip"])
def test_split_inflates_to_the_plain_run(host, cohort, criterion, kind):
    for batch in (1 << 16, 1 << 22):
        tag = "%d_%s_%d" % (criterion, kind, batch)
        d_plain, d_gz = str(cohort["tmp"] / ("sp_" + tag)), str(cohort["tmp"] / ("sz_" + tag))
        counts = _split(host, cohort["paths"][kind], d_plain, criterion, batch, OUT_PLAIN)
        assert _split(host, cohort["paths"][kind], d_gz, criterion, batch, OUT_BGZF) == counts
        names = sorted(os.listdir(d_plain))
        if criterion == SPLIT_CHROMOSOME:
            assert len(names) > 64                                  # files are closed and opened again
        assert sorted(os.listdir(d_gz)) == sorted(n + ".gz" for n in names)
        for n in names:
            packed = open(os.path.join(d_gz, n + ".gz"), "rb").read()
            _walk(packed)                                           # exactly one EOF block, at the end
            assert gzip.decompress(packed) == open(os.path.join(d_plain, n), "rb").read(), (tag, n)
    host.hpgv_run_set_output_compression(OUT_PLAIN)


def test_the_filter_reads_its_own_output(host, cohort):
    tmp = cohort["tmp"]
    a, b = str(tmp / "fb_plain"), str(tmp / "fb_gz")
    _filter(host, cohort["paths"]["bgzip"], a, 1, 1 << 18, OUT_PLAIN)
    _filter(host, cohort["paths"]["bgzip"], b, 1, 1 << 18, OUT_BGZF)
    # the second pass (another threshold would need another setter call: the same filter passes every record again)
    a2, b2 = str(tmp / "fb2_plain"), str(tmp / "fb2_gz")
    c1 = _filter(host, a + ".filtered", a2, 1, 1 << 18, OUT_PLAIN)
    c2 = _filter(host, b + ".filtered.gz", b2, 1, 1 << 18, OUT_PLAIN)
    assert c1 == c2 and c1[0] > 0 and c1[1] == 0
    for ext in (".filtered", ".rejected"):
        assert open(a2 + ext, "rb").read() == open(b2 + ext, "rb").read()


def test_setter_restores_plain_and_refuses_unknown_modes(host, cohort):
    tmp = cohort["tmp"]
    ref, z, back = str(tmp / "set_ref"), str(tmp / "set_z"), str(tmp / "set_back")
    _filter(host, cohort["paths"]["plain"], ref, 1, 1 << 20, OUT_PLAIN)
    _filter(host, cohort["paths"]["plain"], z, 1, 1 << 20, OUT_BGZF)
    assert host.hpgv_run_set_output_compression(7) == hpgv.ERR_INVALID      # refused: the mode stays bgzip
    _filter(host, cohort["paths"]["plain"], z + "2", 1, 1 << 20, None)
    assert os.path.exists(z + "2.filtered.gz") and not os.path.exists(z + "2.filtered")
    _filter(host, cohort["paths"]["plain"], back, 1, 1 << 20, OUT_PLAIN)
    for ext in (".filtered", ".rejected"):
        assert open(back + ext, "rb").read() == open(ref + ext, "rb").read()
        assert not os.path.exists(back + ext + ".gz")
