"""CPU suite: the host mirror's own logic (containers, thread-safe result list,
GT-text staging) built with AddressSanitizer + UBSan and run without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from helpers import QUIRK_GTS, hpgv
from oracle import pyoracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_sources():
    hdir = os.path.join(ROOT, "hpg-variant_amd", "host")
    return [os.path.join(hdir, f) for f in sorted(os.listdir(hdir)) if f.endswith(".c")]


_COMPILED = {}                                       # one build of each kind per session, whichever modules ask for it


def _compile(tmp_path_factory, name, flags):
    if name not in _COMPILED:
        _COMPILED[name] = _compile_once(tmp_path_factory, name, flags)
    return _COMPILED[name]


def _compile_once(tmp_path_factory, name, flags):
    hpgv.build()
    from importlib import import_module
    b = import_module("hpg-variant_amd._build")
    out = str(tmp_path_factory.mktemp("hostcpu") / name)
    # the adapters' source is compiled in directly so that it is instrumented too
    subprocess.check_call(["gcc", "-g", "-std=gnu99", "-fopenmp"] + flags +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "hpg-variant_amd", "host"),
                           os.path.join(ROOT, "tests", "c", "host_cpu_check.c")] + _host_sources() +
                          ["-o", out, "-L", b.LIBDIR, "-lhpgv", "-Wl,-rpath," + b.LIBDIR, "-lm", "-lz", "-lpthread"])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(tmp_path_factory, "host_cpu_check", ["-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


@pytest.fixture(scope="module")
def exe_plain(tmp_path_factory):
    """the shipped optimisation level, no sanitizer: the word-at-a-time staging path (which the ASan build never takes)"""
    return _compile(tmp_path_factory, "host_cpu_check_plain", ["-O2"])


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, env=env)


def test_containers_and_result_list_under_sanitizers(exe):
    r = _run(exe, "containers")
    assert r.returncode == 0 and "CONTAINERS OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


@pytest.mark.parametrize("build", ["asan", "plain"])
def test_staging_matches_the_oracle_encoder(exe, exe_plain, tmp_path, build):
    exe = exe if build == "asan" else exe_plain
    rng = np.random.default_rng(4)
    pool = QUIRK_GTS + ["0/1:12:99", ".:3", "1/", "/1", "0|0:.", "10/2", "a/1", "-1/0", "+1/1", "0/1/2", "2", "<empty>",
                        "./.:0,0", "0/0:1,2:3", "7:1/0", "7:./1:5", "7", "7:"]
    pool += ["1/.", "./1", "1|.", ".|.", "9/9", "0/1:", "0/:", "1/1x", "0/1\t", "./.:", ".", "0", "1:3"]
    hot = ["0/0", "0/1", "1|0", "1/1", "./.", "./1", "1/.", "9/9", "0/1:12:99", "./.:0,0", ".|.", "2/0", "0|9:."]
    long_fmt = ":".join("K%d" % k for k in range(120)) + ":GT"            # > 255 bytes in front of GT (assoc.c:45 strndup's it all)
    fmts = ["GT", "GT:DP", "DP:GT", "DP:GQ:GT", "DP:GQ", "GTX:GT", "XGT", long_fmt]
    chroms = ["1", "X", "XY", "x", "23"]
    n, v = 37, 60
    rows = []
    with open(tmp_path / "in.txt", "w") as f:
        f.write("%d %d\n" % (n, v))
        for i in range(v):
            fmt, chrom = fmts[i % len(fmts)], chroms[i % len(chroms)]
            # two rows in three hold only strings of the hot shape ("a/b", one-character alleles): those rows take the
            # word-at-a-time path of the plain build; a row with any other string is staged the general way
            src = pool if i % 3 == 0 else hot
            ss = [src[int(k)] for k in rng.integers(0, len(src), size=n)]
            f.write("%s %s %s\n" % (chrom, fmt, " ".join(ss)))
            rows.append((chrom, fmt, ss))
    r = _run(exe, "stage", str(tmp_path / "in.txt"))
    assert r.returncode == 0, r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    lines = [l.split() for l in r.stdout.strip().splitlines()]
    assert len(lines) == 2 * v
    for k, t in enumerate(lines):
        strict, i = int(t[0]) == 1, k % v
        chrom, fmt, ss = rows[i]
        assert int(t[1]) == orc.lib().orc_chrom_is_x(chrom.encode(), len(chrom))
        keys = fmt.split(":")
        if "GT" not in keys:
            assert all(x == "ff" for x in t[2:])                     # no GT in FORMAT: nothing usable
            continue
        pos = keys.index("GT")
        exp = ["%02x" % orc.encode_sample("" if s == "<empty>" else s, pos, strict) for s in ss]
        assert t[2:] == exp, (i, strict, list(zip(ss, t[2:], exp)))


@pytest.mark.parametrize("build", ["asan", "plain"])
def test_staging_never_reads_over_a_page_edge(exe, exe_plain, build):
    r = _run(exe if build == "asan" else exe_plain, "pageedge")
    assert r.returncode == 0 and "PAGEEDGE OK" in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


@pytest.mark.parametrize("build", ["asan", "plain"])
def test_record_head_store_grows_and_reads_back(exe, exe_plain, build):
    # rec_heads_* (what .mperm and .clumped keep "CHR\tPOS\tID" of their records in): 70 000 records from a first capacity of 4,
    # the arena doubling from 64 KiB to 16 MiB, read back one by one; a first record longer than 64 KiB; the free of an unused
    # store.  The sanitised build runs with its leak check on: what rec_heads_free leaves behind fails the run at exit
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe if build == "asan" else exe_plain, "heads"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "HEADS OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


_HDR_ASSOC = "#CHR\tPOS\tID\tA1\tC_A1\tC_U1\tF_A1\tF_U1\tA2\tC_A2\tC_U2\tF_A2\tF_U2\tOR\t%sP-VALUE"
_HDR = {
    "chisq": _HDR_ASSOC % "CHISQ\t", "fisher": _HDR_ASSOC % "", "tdt": "#CHR\tPOS\tID\tA1\tA2\tT\tU\tOR\tCHISQ\tP-VALUE",
    "model": "#CHR\tPOS\tID\tA1\tA2\tAFF\tUNAFF\tCHISQ_GENO\tP_GENO\tCHISQ_TREND\tP_TREND\tCHISQ_ALLELIC\tP_ALLELIC\tCHISQ_DOM\tP_DOM\tCHISQ_REC\tP_REC",
    "logistic": "#CHR\tPOS\tID\tA1\tA2\tNOBS\tBETA\tSE\tOR\tSTAT\tP\tITER", "linear": "#CHR\tPOS\tID\tA1\tA2\tNOBS\tBETA\tSE\tSTAT\tP",
}
# The tools' traits, written out a second time on purpose: an edit to a row of the table in hpgv_host_internal.h has to be made here too.
# number, name: (cohort stage, covariates, PED required, takes hpgv_run_set_record_filters, sorted afterwards, .mperm, stats counters,
# per-record lines, sample-pair buffers, the tool whose file it writes, ints per line, doubles per line)
_TRAITS = {
    (1, "chisq"): ("case-control", 0, 1, 1, 1, 0, 0, 1, 0, "chisq", 4, 3),
    (2, "fisher"): ("case-control", 0, 1, 1, 1, 0, 0, 1, 0, "fisher", 4, 3),
    (3, "tdt"): ("families", 0, 1, 1, 1, 0, 0, 1, 0, "tdt", 4, 3),
    (4, "vcf2epi"): ("case-control", 0, 1, 1, 0, 0, 0, 1, 0, "vcf2epi", 4, 3),
    (5, "aggregate"): ("columns", 0, 0, 1, 0, 0, 1, 1, 0, "aggregate", 4, 3),
    (6, "stats"): ("columns", 0, 0, 0, 0, 0, 1, 1, 0, "stats", 4, 3),
    (7, "filter"): ("columns", 0, 0, 1, 0, 0, 0, 0, 0, "filter", 4, 3),
    (8, "split"): ("columns", 0, 0, 0, 0, 0, 0, 0, 0, "split", 4, 3),
    (9, "chisq_perm"): ("case-control", 0, 1, 1, 1, 1, 0, 1, 0, "chisq", 4, 3),
    (10, "tdt_perm"): ("families", 0, 1, 1, 1, 1, 0, 1, 0, "tdt", 4, 3),
    (11, "model"): ("case-control", 0, 1, 1, 1, 0, 0, 1, 0, "model", 8, 10),
    (12, "model_perm"): ("case-control", 0, 1, 1, 1, 1, 0, 1, 0, "model", 8, 10),
    (13, "genome"): ("columns", 0, 0, 0, 0, 0, 0, 0, 1, "genome", 4, 3),
    (14, "grm"): ("columns", 0, 0, 0, 0, 0, 0, 0, 1, "grm", 4, 3),
    (15, "logistic"): ("case-control", 1, 1, 1, 1, 0, 0, 1, 0, "logistic", 4, 6),
    (16, "linear"): ("trait", 1, 0, 1, 1, 0, 0, 1, 0, "linear", 4, 6),
}


@pytest.mark.parametrize("build", ["asan", "plain"])
def test_tool_traits_table_and_batch_arrays_at_every_width(exe, exe_plain, build):
    # the table row by row against the copy above, its derived properties against their definitions, and every tool's per-line
    # arrays written through at the table's widths before and after they are rebuilt (host_cpu_check.c: cmd_traits)
    r = _run(exe if build == "asan" else exe_plain, "traits")
    assert r.returncode == 0 and "TRAITS OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    got = {}
    for line in r.stdout.splitlines():
        if not line.startswith("tool "):
            continue
        head, header = line.split(" header=")
        f = head.split(" ")
        kv = dict(x.split("=") for x in f[3:])
        row = (kv["cohort"],) + tuple(int(kv[k]) for k in ("covar", "ped", "rec_filters", "sorts", "mperm", "counts", "lines", "pairs")) \
            + (kv["file"], int(kv["ints"]), int(kv["dbls"]))
        got[(int(f[1]), f[2])] = row
        assert int(kv["installs"]) == (row[0] in ("case-control", "trait")), line      # installs the assoc cohort itself
        assert int(kv["writer"]) == (row[4] or row[6]), line                           # its lines may go through the writer thread
        assert header == (_HDR[row[9]] if row[4] else "-"), line                       # a header kept for the order check: the sorted tools
    assert got == _TRAITS
    assert sum(l.startswith("PASS ") for l in r.stdout.splitlines()) == len(_TRAITS)


def test_in_process_sort_equals_gnu_sort(exe, tmp_path):
    # assoc_runner.c:255-258 shells out to `sort -k1,1h -k2,2n`; the in-process replacement must give
    # the same file (C locale), header line included
    rng = np.random.default_rng(12)
    chroms = [str(c) for c in range(1, 23)] + ["X", "Y", "MT", "chr1", "1_KI270706v1_random", "GL000192.1", "10", "010", "2K"]
    lines = ["#CHR\tPOS\tID\tA1\tA2\tT\tU\tOR\tCHISQ\tP-VALUE"]
    for i in range(3000):
        c = chroms[int(rng.integers(0, len(chroms)))]
        pos = int(rng.integers(1, 5000)) if i % 10 else int(rng.integers(1, 250_000_000))
        lines.append("%s\t%d\trs%d\tA\tC\t%d\t%d\t%6f\t%6f\t%6f" % (c, pos, int(rng.integers(0, 50)), i % 7, i % 5, 1.5, 2.25, 0.125))
    order = rng.permutation(len(lines))
    body = "\n".join(lines[i] for i in order) + "\n"
    a, b = tmp_path / "mine.tsv", tmp_path / "gnu_in.tsv"
    a.write_text(body); b.write_text(body)
    r = _run(exe, "sort", str(a))
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr, r.stderr
    env = dict(os.environ, LC_ALL="C")
    gnu = subprocess.run(["sort", "-k1,1h", "-k2,2n", str(b)], capture_output=True, text=True, env=env, check=True).stdout
    assert a.read_text() == gnu
    assert a.read_text().splitlines()[0].startswith("#CHR") or "X" in chroms      # header sorts with the text keys


def _bgzf(data, block=0xff00):
    """BGZF as bgzip writes it: gzip members with a 'BC' extra field holding the block size, then the
    28-byte end-of-file marker."""
    import struct
    import zlib
    out = bytearray()
    chunks = [data[i:i + block] for i in range(0, len(data), block)] + [b""]
    for ch in chunks:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = co.compress(ch) + co.flush()
        bsize = 12 + 6 + len(comp) + 8
        out += b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6)
        out += b"BC" + struct.pack("<HH", 2, bsize - 1) + comp + struct.pack("<II", zlib.crc32(ch), len(ch))
    return bytes(out)


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf"])
@pytest.mark.parametrize("header", [False, True])
@pytest.mark.parametrize("batch", [1 << 16, 200_000, 1 << 22])
def test_line_reader_sources(exe, tmp_path, kind, batch, header):
    # --compression gzip|bgzip (shared_options.c:60-61): every source hands out the same bytes in whole lines
    import gzip
    rng = np.random.default_rng(7)
    lines = []
    for i in range(9000):
        n = int(rng.integers(0, 300)) if i % 50 else int(rng.integers(20_000, 60_000))
        lines.append(bytes(rng.integers(48, 58, size=n, dtype=np.uint8)) + b"\n")
    data = b"".join(lines)[:-1]                                      # the last line has no newline
    head = b""
    if header:                                                       # the runners take the header off first; what
        head = b"##fileformat=VCFv4.1\n" + b"##x=" + b"y" * 100_000 + b"\n"          # was read past it is carried over
        head += b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + b"\t".join(b"s%d" % i for i in range(3000)) + b"\n"
    src = tmp_path / "in"
    full = head + data
    src.write_bytes({"plain": full, "gzip": gzip.compress(full, 1), "bgzf": _bgzf(full)}[kind])
    r = _run(exe, "copy", str(src), str(tmp_path / "out"), str(batch), *(["vcf"] if header else []))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert (tmp_path / "out").read_bytes() == data
    assert int(r.stdout.split()[-1]) >= len(data) // batch


def test_line_reader_rejects_damaged_bgzf(exe, tmp_path):
    data = b"".join(b"%d\n" % i for i in range(200_000))
    blob = bytearray(_bgzf(data))
    blob[len(blob) // 2] ^= 0x55
    (tmp_path / "in").write_bytes(bytes(blob))
    r = _run(exe, "copy", str(tmp_path / "in"), str(tmp_path / "out"), str(1 << 20))
    assert r.returncode != 0
    assert "AddressSanitizer" not in r.stderr, r.stderr


@pytest.mark.parametrize("kind", ["plain", "bgzf"])
def test_line_reader_header_longer_than_its_buffer(exe, tmp_path, kind):
    head = b"##big=" + b"z" * (5 << 20) + b"\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\n"
    data = b"".join(b"1\t%d\trs\tA\tC\t.\t.\t.\tGT\t0/1\t1/1\n" % i for i in range(50_000))
    (tmp_path / "in").write_bytes(head + data if kind == "plain" else _bgzf(head + data))
    r = _run(exe, "copy", str(tmp_path / "in"), str(tmp_path / "out"), str(1 << 18), "vcf")
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
    assert (tmp_path / "out").read_bytes() == data
    (tmp_path / "nohdr").write_bytes(data)
    assert _run(exe, "copy", str(tmp_path / "nohdr"), str(tmp_path / "out2"), str(1 << 18), "vcf").returncode != 0


def test_deflate_decoder_against_zlib_under_sanitizers(exe):
    # hpgv_host_inflate_raw (the bgzip reader's decoder): 750 valid streams (text, incompressible, runs, every zlib strategy
    # incl. fixed codes and stored blocks, sizes 0 .. 1 MiB) decode to the original; damaged / truncated streams and wrong
    # output sizes are refused or decoded without any access outside the buffers
    r = _run(exe, "inflate")
    assert r.returncode == 0 and "inflate ok" in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def _bgzf_stored(ch):
    """one BGZF block holding `ch` uncompressed (deflate level 0)"""
    import struct
    import zlib
    co = zlib.compressobj(0, zlib.DEFLATED, -15)
    comp = co.compress(ch) + co.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(comp) + 8 - 1)
            + comp + struct.pack("<II", zlib.crc32(ch), len(ch)))


def _walk_bgzf(blob):
    """(blocks, text bytes) of a well-formed BGZF file, from its headers' BC fields and its trailers' ISIZE"""
    pos = n = text = 0
    while pos < len(blob):
        assert blob[pos:pos + 4] == b"\x1f\x8b\x08\x04"
        off, bsize = pos + 12, None
        end = off + int.from_bytes(blob[pos + 10:pos + 12], "little")
        while off + 4 <= end:
            slen = int.from_bytes(blob[off + 2:off + 4], "little")
            if blob[off:off + 2] == b"BC" and slen == 2:
                bsize = int.from_bytes(blob[off + 4:off + 6], "little") + 1
            off += 4 + slen
        text += int.from_bytes(blob[pos + bsize - 4:pos + bsize], "little")
        pos += bsize
        n += 1
    assert pos == len(blob)
    return n, text


def test_block_table_team_walk_equals_serial_walk(exe, tmp_path):
    # the table the device path's stager takes its rows from when the host builds it: by the team (64 segments, pread) and by
    # one thread (the mapping), row for row the same, and the same block count and text length as a walk of the file here
    rng = np.random.default_rng(19)
    data = bytes(rng.integers(48, 58, size=1_500_000, dtype=np.uint8))
    even = _bgzf(data)
    assert len(even) >= 64 * 4096                                    # under that the team leaves the file to the serial walk
    # blocks of very different sizes: a stored 64 KB block spans more than two of the 64 segments, so some hold no block start
    n_big, big = 10, 0xfe00
    mixed = b"".join(_bgzf_stored(data[i * big:(i + 1) * big]) for i in range(n_big)) + _bgzf(data[n_big * big:n_big * big + 300 * 0x700], 0x700)
    assert len(mixed) >= 64 * 4096 and len(mixed) // 64 < big // 2
    for tag, blob in (("even", even), ("mixed", mixed)):
        (tmp_path / tag).write_bytes(blob)
        r = _run(exe, "blocktable", str(tmp_path / tag))
        assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        last = r.stdout.strip().splitlines()[-1].split()
        assert last[0] == "blocktable" and (int(last[1]), int(last[2])) == _walk_bgzf(blob), (tag, last)
        assert "serial only" not in r.stdout, tag                    # both files are over the team's floor: it must take them
        assert "team walk and serial walk give the same rows" in r.stdout
    cut = even[:len(even) * 2 // 3 + 5]                              # cut off inside a block: neither walk takes it
    assert len(cut) >= 64 * 4096
    (tmp_path / "cut").write_bytes(cut)
    r = _run(exe, "blocktable", str(tmp_path / "cut"))
    assert r.returncode == 1 and "blocktable refused" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
