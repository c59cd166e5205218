#!/usr/bin/env python3
"""The filter tool's numbers (DESIGN.md "Partition of lines"):
  kernel   hpgv_lines_partition_dev on 256 MB of lines of 10 000 samples (~40 KB) and of 200 samples (~800 B), every other
           line kept: wall time per call over --iters calls, and the rate (bytes read + written) / time as a share of the
           8 TB/s HBM peak.  Under `rocprofv3 --kernel-trace --stats` (a run of its own) the kernel's own time.
  run      hpgv_run_filter with save_rejected = 1 (every record written: the input's record bytes) on a 10 000-sample file,
           plain and bgzip, half the records kept by --quality; next to hpgv_host_copy_lines on the same file (the reader
           alone writing every line).  Wall and stage times.
One JSON line per measurement.  HPGV_LIB=<ablation build> with --aligned-loads: the aligned-loads + v_alignbyte form."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib
import struct
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hpgv = import_module("hpg-variant_amd")
HBM_PEAK = 8.0e12


def lines_of(n_samples, total, rng):
    line = ("1\t100\trs1\tA\tC\t50\tPASS\t.\tGT" + "\t0/1" * n_samples + "\n").encode()
    n = max(1, total // len(line))
    jitter = rng.integers(0, 16, n)                               # lengths differ a little: every alignment occurs
    lens = len(line) + jitter
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    text = np.frombuffer(rng.bytes(int(off[-1])), np.uint8).copy()
    text[(off[1:] - 1).astype(np.int64)] = 10
    return text, off


def bench_kernel(args, L, ctx, n_samples):
    rng = np.random.default_rng(n_samples)
    text, off = lines_of(n_samples, args.mb << 20, rng)
    n = len(off) - 1
    keep = (np.arange(n) % 2).astype(np.uint8)
    vp = C.c_void_p
    bufs = []

    def alloc(b):
        p = vp()
        assert L.hpgv_dev_alloc(ctx, b, C.byref(p)) == 0
        bufs.append(p)
        return p.value

    d_text, d_off, d_keep = alloc(text.nbytes + 16), alloc(off.nbytes), alloc(n)
    d_out, d_kept = alloc(text.nbytes + 16), alloc(8)
    d_scr = alloc(L.hpgv_lines_partition_scratch_bytes(n))
    for d, a in ((d_text, text), (d_off, off), (d_keep, keep)):
        assert L.hpgv_memcpy_h2d(ctx, d, a.ctypes.data, a.nbytes, None) == 0
    if args.aligned_loads:
        assert L.hpgv_set_option(ctx, b"part_aligned_loads", 1) == 0, L.hpgv_last_error(ctx)
    call = lambda: L.hpgv_lines_partition_dev(ctx, d_text, d_off, n, d_keep, d_out + 3, d_kept, d_scr, None)
    for _ in range(3):
        assert call() == 0
    assert L.hpgv_stream_sync(ctx, None) == 0
    t0 = time.perf_counter()
    for _ in range(args.iters):
        call()
    assert L.hpgv_stream_sync(ctx, None) == 0
    dt = (time.perf_counter() - t0) / args.iters
    got = np.empty(text.nbytes, np.uint8)
    assert L.hpgv_memcpy_d2h(ctx, got.ctypes.data, d_out + 3, got.nbytes, None) == 0
    ks = [slice(int(off[i]), int(off[i + 1])) for i in range(n)]
    exp = np.concatenate([text[s] for i, s in enumerate(ks) if keep[i]] + [text[s] for i, s in enumerate(ks) if not keep[i]])
    assert np.array_equal(got, exp)
    for p in bufs:
        L.hpgv_dev_free(ctx, p)
    moved = 2.0 * text.nbytes
    print(json.dumps({"what": "partition_kernel", "samples": n_samples, "lines": n, "bytes": int(text.nbytes),
                      "aligned_loads": bool(args.aligned_loads), "ms_per_call": round(dt * 1e3, 4),
                      "gbps": round(moved / dt / 1e9, 1), "share_of_hbm_peak": round(moved / dt / HBM_PEAK, 3)}), flush=True)


def bgzf(data, block=0xff00):
    """BGZF as bgzip writes it (level 1 here), with the end-of-file block"""
    out = bytearray()
    for ch in [data[i:i + block] for i in range(0, len(data), block)] + [b""]:
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        comp = co.compress(ch) + co.flush()
        bsize = 12 + 6 + len(comp) + 8
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1) + comp
        out += struct.pack("<II", zlib.crc32(ch), len(ch))
    return bytes(out)


def bench_run(args, n_samples):
    H = C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)

    class F(C.Structure):
        _fields_ = [("min_maf", C.c_double), ("max_missing", C.c_double), ("max_mendel_errors", C.c_int),
                    ("num_alleles", C.c_int), ("min_quality", C.c_double)]
    H.hpgv_run_filter.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    H.hpgv_run_set_filters.argtypes = [C.POINTER(F)]
    H.hpgv_host_copy_lines.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_long)]
    H.hpgv_host_last_error.restype = C.c_char_p
    os.makedirs(args.workdir, exist_ok=True)
    rec = "\t0/1" * n_samples + "\n"
    n_rec = max(2, (args.run_mb << 20) // (len(rec) + 40))
    hdr = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + "".join("\ts%d" % j for j in range(n_samples)) + "\n"
    body = "".join("1\t%d\trs%d\tA\tC\t%d\tPASS\t.\tGT%s" % (100 + v, v, 10 if v % 2 else 50, rec) for v in range(n_rec))
    data = (hdr + body).encode()
    paths = {"plain": os.path.join(args.workdir, "f.vcf"), "bgzip": os.path.join(args.workdir, "f.vcf.gz")}
    with open(paths["plain"], "wb") as f:
        f.write(data)
    with open(paths["bgzip"], "wb") as f:
        f.write(bgzf(data))
    t = (C.c_double * 6)()
    for kind, path in paths.items():
        for rep in range(2):                                       # the first run warms the page cache and the engine
            fl = F(-1, -1, -1, -1, 30.0)
            H.hpgv_run_set_filters(C.byref(fl))
            a, r = C.c_long(0), C.c_long(0)
            t0 = time.perf_counter()
            rc = H.hpgv_run_filter(path.encode(), None, os.path.join(args.workdir, "out").encode(), 1, 1 << 26, C.byref(a), C.byref(r))
            wall = time.perf_counter() - t0
            H.hpgv_run_set_filters(None)
            assert rc == 0, H.hpgv_host_last_error()
            H.hpgv_host_last_run_times(t)
            nb = C.c_long(0)
            t0 = time.perf_counter()
            rc = H.hpgv_host_copy_lines(path.encode(), os.path.join(args.workdir, "copy").encode(), 1 << 26, 1, C.byref(nb))
            copy = time.perf_counter() - t0
            assert rc == 0
        print(json.dumps({"what": "filter_run", "input": kind, "samples": n_samples, "records": n_rec, "text_bytes": len(data),
                          "kept": a.value, "rejected": r.value, "wall_s": round(wall, 4),
                          "stages_s": {"read": round(t[0], 4), "engine": round(t[1], 4), "write": round(t[2], 4), "total": round(t[4], 4)},
                          "batches": int(t[5]), "copy_lines_s": round(copy, 4), "ratio_to_copy_lines": round(wall / copy, 3)}), flush=True)
    for p in list(paths.values()) + [os.path.join(args.workdir, x) for x in ("out.filtered", "out.rejected", "copy")]:
        if os.path.exists(p):
            os.remove(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256, help="MB of lines per kernel call")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--aligned-loads", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--run-mb", type=int, default=512, help="MB of text of the whole-run file")
    ap.add_argument("--workdir", default="/tmp/hpgv_bench_filter")
    args = ap.parse_args()
    L = hpgv.load()
    L.hpgv_lines_partition_scratch_bytes.argtypes = [C.c_int]
    L.hpgv_lines_partition_scratch_bytes.restype = C.c_size_t
    L.hpgv_lines_partition_dev.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 5
    ctx = C.c_void_p()
    assert L.hpgv_create(0, C.byref(ctx)) == 0
    for ns in (10000, 200):
        bench_kernel(args, L, ctx, ns)
    L.hpgv_destroy(ctx)
    if not args.kernel_only:
        bench_run(args, 10000)


if __name__ == "__main__":
    main()
