"""CPU suite: the C-ABI libraries load and export every symbol the headers
declare (no compute calls: there is no GPU here), the product fails loudly
without a device, and the oracle is not reachable from the product."""
import ctypes as C
import os
import re
import subprocess

import pytest

from helpers import hpgv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b([a-z_][a-z0-9_]*)\s*\((?!\*)", text))
    return sorted(names - {"defined", "sizeof", "void", "int", "char"})


@pytest.fixture(scope="module", autouse=True)
def built():
    hpgv.build()


def test_libhpgv_exports_every_declared_symbol():
    L = hpgv.load()
    names = [n for n in _declared("hpgv.h") if n.startswith("hpgv_")]
    assert set(names) == set(hpgv.SYMBOLS), set(names) ^ set(hpgv.SYMBOLS)
    for n in names:
        assert hasattr(L, n), n


def test_libhpgv_host_exports_reference_api():
    from importlib import import_module
    b = import_module("hpg-variant_amd._build")
    L = C.CDLL(b.HOSTLIB)
    names = [n for n in _declared("hpgv_host.h") if not n.startswith("pthread")]
    for n in names:
        assert hasattr(L, n), n
    # the three per-batch entry points of the reference are there by name
    for n in ("assoc_test", "tdt_test", "get_variants_stats", "init_logarithm_array"):
        assert n in names


def test_no_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(hpgv.HpgvError) as e:
        hpgv.Engine(0)
    assert "no CPU fallback" in str(e.value)


def test_rccl_loader_survives_a_wrong_library_path():
    """a candidate that fails to dlopen (a wrong HPGV_RCCL_LIB) must end in the fallback names or in
    HPGV_ERR_UNSUPPORTED with the loader's text -- never in a crash.  Own process: a segfault would take pytest down."""
    code = ("import importlib, ctypes as C, sys; sys.path.insert(0, %r); h = importlib.import_module('hpg-variant_amd'); "
            "L = h.load(); b = C.create_string_buffer(2048); rc = L.hpgv_group_rccl_probe(b, 2048); "
            "print(rc, b.value.decode()); sys.exit(0 if rc in (h.OK, h.ERR_UNSUPPORTED) else 3)" % ROOT)
    for lib in ("/nonexistent/librccl.so", ""):
        env = dict(os.environ, HPGV_RCCL_LIB=lib)
        r = subprocess.run([os.sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        if lib:
            assert "/nonexistent/librccl.so" in r.stdout      # the failed candidate is named in the message


def test_rccl_probe_accepts_the_stand_in_communicator(tmp_path):
    """tests/c/fake_rccl.hip, built as the GPU tests' fixture builds it, offers every symbol the group scan resolves
    (RCCL_SYMBOLS) and exports nothing else: hpgv_group_rccl_probe with HPGV_RCCL_LIB set to it says HPGV_OK.  Own process:
    the environment is the child's."""
    from helpers import build_fake_rccl
    lib, names = build_fake_rccl(tmp_path)
    assert len(names) == 9
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in exported.splitlines() if line.strip()) == sorted(names)
    code = ("import importlib, ctypes as C, sys; sys.path.insert(0, %r); h = importlib.import_module('hpg-variant_amd'); "
            "L = h.load(); b = C.create_string_buffer(2048); rc = L.hpgv_group_rccl_probe(b, 2048); "
            "print(rc, b.value.decode()); sys.exit(0 if rc == h.OK else 3)" % ROOT)
    r = subprocess.run([os.sys.executable, "-c", code], env=dict(os.environ, HPGV_RCCL_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    # one symbol short, and the probe says so (the loader falls through to no other candidate: the file itself loads)
    short = str(tmp_path / "libshort.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-x", "c", "-o", short, "-"], input=b"int ncclSend(void) { return 0; }\n", check=True)
    r = subprocess.run([os.sys.executable, "-c", code], env=dict(os.environ, HPGV_RCCL_LIB=short), capture_output=True, text=True, timeout=300)
    assert r.returncode == 3 and r.stdout.startswith("%d" % hpgv.ERR_UNSUPPORTED), (r.returncode, r.stdout, r.stderr)


def test_product_does_not_link_or_import_the_oracle():
    pkg = os.path.join(ROOT, "hpg-variant_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".c", ".h", ".hip", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not re.search(r'#\s*include\s*[<"][^>"]*oracle', src), f
                assert not re.search(r"^\s*(from|import)\s+\S*oracle", src, flags=re.M), f
                assert "orc_" not in re.sub(r"//.*|/\*.*?\*/", "", src, flags=re.S), f
    from importlib import import_module
    b = import_module("hpg-variant_amd._build")
    for lib in (b.LIB, b.HOSTLIB):
        out = subprocess.run(["ldd", lib], capture_output=True, text=True).stdout
        assert "oracle" not in out


def test_status_codes_and_enums_match_header():
    text = open(os.path.join(ROOT, "include", "hpgv.h")).read()
    assert "HPGV_TASK_CHISQ = 1" in text and hpgv.TASK_CHISQ == 1
    assert "HPGV_TASK_FISHER = 2" in text and hpgv.TASK_FISHER == 2
    assert "HPGV_COND_AFFECTED = 1" in text and hpgv.COND_AFFECTED == 1
    assert "HPGV_SEX_MALE = 0" in text and hpgv.SEX_MALE == 0


def test_tile_record_constants_match_the_kernels_header():
    # the layout of the tokenizer's tile records that the package gives the tests, against csrc/hpgv_text2_kernels.h and hpgv.h
    text = open(os.path.join(ROOT, "hpg-variant_amd", "csrc", "hpgv_text2_kernels.h")).read()
    assert re.search(r"struct TokAgg \{ int nl, tabs, last_nl, pad; \};", text)
    assert (hpgv.TOK_AGG_NL, hpgv.TOK_AGG_TABS, hpgv.TOK_AGG_LAST_NL, hpgv.TOK_AGG_PAD) == (0, 1, 2, 3) and hpgv.TOK_TILE_HALF_WORDS == 4
    assert re.search(r"struct TokAgg2 \{ TokAgg h\[2\]; \};", text) and hpgv.TOK_TILE_RECORD_BYTES == 2 * 4 * hpgv.TOK_TILE_HALF_WORDS
    m = re.search(r"enum \{ TOK_AGG_WRITTEN = (\d+), TOK_AGG_COMPLEX = (\d+) \};", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (hpgv.TOK_AGG_WRITTEN, hpgv.TOK_AGG_COMPLEX)
    tb = int(re.search(r"constexpr int TOK2_TB = (\d+);", text).group(1))
    threads = int(re.search(r"#define HPGV_TOK2_THREADS (\d+)", text).group(1))
    assert re.search(r"constexpr int TOK2_TILE = TOK2_THREADS \* TOK2_TB;", text) and tb * threads == hpgv.TOK_TILE_BYTES
    L = hpgv.load()
    for n in (0, 1, 2048, 2049, 600_000):                           # one record per tile and one to spare
        assert L.hpgv_text_tiles_bytes(n) == ((n + hpgv.TOK_TILE_BYTES - 1) // hpgv.TOK_TILE_BYTES + 1) * hpgv.TOK_TILE_RECORD_BYTES


def test_format_f6_is_printf_percent_6f():
    # the writers' own "%6f" (hpgv_host_format_f6) against libc's snprintf, character for character: random doubles of every
    # magnitude, exact ties of the sixth decimal (j / 128 -> ...5 exactly), the fall-back range, denormals, signed zeros, NaN, inf
    import ctypes.util
    import struct
    import numpy as np
    from importlib import import_module
    b = import_module("hpg-variant_amd._build")
    H = C.CDLL(b.HOSTLIB)
    H.hpgv_host_format_f6.argtypes = [C.c_double, C.c_char_p]
    H.hpgv_host_format_f6.restype = C.c_int
    libc = C.CDLL(ctypes.util.find_library("c"))
    libc.snprintf.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_double]
    rng = np.random.default_rng(6)
    xs = [0.0, -0.0, 1.0, -1.0, 0.5, 1e-7, 5e-7, 4.999999e-7, 2.5e-6, 0.0078125, 0.0234375, 1 / 128, 3 / 128, 5 / 128, 255 / 128,
          0.9999995, 0.99999949999, 0.9999994999999999, 123456.7890125, 8.9999e12, 9e12, 9.0000001e12, 1e15, 1e300, -1e300,
          5e-324, 2.2250738585072014e-308, float("inf"), float("-inf"), float("nan"), -float("nan"), 16.666666666666668, 4.4557090604024907e-05]
    xs += [j / 128.0 + k for j in range(1, 128, 2) for k in (0, 7, 1024)]                    # ties: ....5 exactly in binary
    xs += list(rng.random(20000))                                                           # p-values, frequencies
    xs += list(rng.random(5000) * 10.0 ** rng.integers(-12, 13, 5000))                       # every magnitude below 1e13
    xs += [struct.unpack("<d", struct.pack("<Q", int(v)))[0] for v in rng.integers(0, 2 ** 63, 20000, dtype=np.uint64) * 2 + rng.integers(0, 2, 20000, dtype=np.uint64)]
    got, exp = C.create_string_buffer(512), C.create_string_buffer(512)
    for x in xs:
        n = H.hpgv_host_format_f6(x, got)
        libc.snprintf(exp, 512, b"%6f", C.c_double(x))
        assert got.value == exp.value and n == len(exp.value), (x, got.value, exp.value)
