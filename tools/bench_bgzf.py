#!/usr/bin/env python3
"""The bgzip output's numbers (DESIGN.md "BGZF written on the device"):
  kernel   hpgv_bgzf_deflate_dev on --mb MB of genotype lines of 10 000 and of 200 samples (d/d, d|d, ./. drawn per line with
           a random allele frequency), one segment: wall time per call over --iters calls and text bytes in per second; the
           size of the members next to zlib level 1 and zlib level 1 Z_FIXED on the same 65 280-byte blocks (a sample of them).
           Under `rocprofv3 --kernel-trace --stats` (a run of its own) the kernels' own times, the compaction copy apart.
  run      hpgv_run_filter (save_rejected = 1) and hpgv_run_split by chromosome on the 10 000-sample file of bench_filter.py /
           bench_split.py, plain and bgzip input, HPGV_OUT_PLAIN against HPGV_OUT_BGZF: stage times of --reps runs each.
One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import time
import zlib
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hpgv = import_module("hpg-variant_amd")
from bench_filter import bgzf                                     # noqa: E402

BLOCK = 65280


def genotype_lines(n_samples, total, rng):
    codes = np.array([b"0/0", b"0/1", b"1/0", b"1/1", b"0|0", b"0|1", b"1|0", b"1|1", b"./."])
    out, size, v = [], 0, 0
    while size < total:
        af = rng.random() * 0.5
        p_a = np.array([(1 - af) ** 2, af * (1 - af), af * (1 - af), af * af])
        p = np.concatenate([p_a * 0.49, p_a * 0.49, [0.02]])
        line = b"%d\t%d\trs%d\tA\tC\t50\tPASS\t.\tGT\t" % (1 + v % 22, 1000 + 7 * v, v) + b"\t".join(codes[rng.choice(9, size=n_samples, p=p)]) + b"\n"
        out.append(line); size += len(line); v += 1
    return b"".join(out)[:total]


def bench_kernel(args, L, ctx, n_samples):
    text = genotype_lines(n_samples, args.mb << 20, np.random.default_rng(n_samples))
    n = len(text)
    bufs = []

    def alloc(b):
        p = C.c_void_p()
        assert L.hpgv_dev_alloc(ctx, b, C.byref(p)) == 0
        bufs.append(p)
        return p.value

    d_text, d_seg, d_so = alloc(n + 16), alloc(16), alloc(16)
    d_out, d_scr = alloc(L.hpgv_bgzf_deflate_bound(n, 1)), alloc(L.hpgv_bgzf_deflate_scratch_bytes(n, 1))
    arr = np.frombuffer(text, np.uint8)
    seg = np.array([0, n], np.uint64)
    assert L.hpgv_memcpy_h2d(ctx, d_text, arr.ctypes.data, n, None) == 0 and L.hpgv_memcpy_h2d(ctx, d_seg, seg.ctypes.data, 16, None) == 0
    call = lambda: L.hpgv_bgzf_deflate_dev(ctx, d_text, d_seg, 1, d_out, d_so, d_scr, None)
    for _ in range(2):
        assert call() == 0, L.hpgv_last_error(ctx)
    assert L.hpgv_stream_sync(ctx, None) == 0
    t0 = time.perf_counter()
    for _ in range(args.iters):
        call()
    assert L.hpgv_stream_sync(ctx, None) == 0
    dt = (time.perf_counter() - t0) / args.iters
    so = np.zeros(2, np.uint64)
    assert L.hpgv_memcpy_d2h(ctx, so.ctypes.data, d_so, 16, None) == 0
    made = int(so[1])
    sample = range(0, n, BLOCK * max(1, n // BLOCK // 256))           # every k-th block: 256 of them
    z1 = zf = raw = 0
    for at in sample:
        blk = text[at:at + BLOCK]
        a = zlib.compressobj(1, zlib.DEFLATED, -15); b = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
        z1 += len(a.compress(blk) + a.flush()) + 26; zf += len(b.compress(blk) + b.flush()) + 26; raw += len(blk)
    for p in bufs:
        L.hpgv_dev_free(ctx, p)
    print(json.dumps({"what": "deflate_kernel", "samples": n_samples, "text_bytes": n, "member_bytes": made, "ms_per_call": round(dt * 1e3, 3),
                      "text_gbps": round(n / dt / 1e9, 1), "ratio": round(made / n, 4), "ratio_zlib1": round(z1 / raw, 4),
                      "ratio_zlib1_fixed": round(zf / raw, 4)}), flush=True)


def bench_runs(args):
    H = C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)

    class F(C.Structure):
        _fields_ = [("min_maf", C.c_double), ("max_missing", C.c_double), ("max_mendel_errors", C.c_int),
                    ("num_alleles", C.c_int), ("min_quality", C.c_double)]
    H.hpgv_run_filter.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    H.hpgv_run_split.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t] + [C.POINTER(C.c_long)] * 3
    H.hpgv_run_set_filters.argtypes = [C.POINTER(F)]
    H.hpgv_host_last_error.restype = C.c_char_p
    os.makedirs(args.workdir, exist_ok=True)
    n_samples = 10000
    rec = "\t0/1" * n_samples + "\n"
    n_rec = max(2, (args.run_mb << 20) // (len(rec) + 40))
    hdr = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + "".join("\ts%d" % j for j in range(n_samples)) + "\n"
    body = "".join("%d\t%d\trs%d\tA\tC\t%d\tPASS\t.\tGT%s" % (1 + v * 24 // n_rec, 100 + v, v, 10 if v % 2 else 50, rec) for v in range(n_rec))
    data = (hdr + body).encode()
    paths = {"plain": os.path.join(args.workdir, "f.vcf"), "bgzip": os.path.join(args.workdir, "f.vcf.gz")}
    open(paths["plain"], "wb").write(data)
    open(paths["bgzip"], "wb").write(bgzf(data))
    t = (C.c_double * 6)()
    for tool in ("filter", "split"):
        for kind, path in paths.items():
            for mode in (0, 1):
                assert H.hpgv_run_set_output_compression(mode) == 0
                rows = []
                for rep in range(args.reps + 1):                   # the first run warms the page cache and the engine
                    out = os.path.join(args.workdir, "out_" + tool)
                    shutil.rmtree(out, ignore_errors=True)
                    a, r, s = C.c_long(0), C.c_long(0), C.c_long(0)
                    if tool == "filter":
                        fl = F(-1, -1, -1, -1, 30.0)
                        H.hpgv_run_set_filters(C.byref(fl))
                        rc = H.hpgv_run_filter(path.encode(), None, out.encode(), 1, 1 << 26, C.byref(a), C.byref(r))
                        H.hpgv_run_set_filters(None)
                    else:
                        rc = H.hpgv_run_split(path.encode(), out.encode(), 1, None, 0, 1 << 26, C.byref(a), C.byref(r), C.byref(s))
                    assert rc == 0, H.hpgv_host_last_error()
                    H.hpgv_host_last_run_times(t)
                    if rep:
                        rows.append([round(t[0], 4), round(t[1], 4), round(t[2], 4), round(t[4], 4)])
                written = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(args.workdir) for f in fs if f.startswith("out_") or "out_" in dp)
                print(json.dumps({"what": tool + "_run", "input": kind, "output": "bgzf" if mode else "plain", "text_bytes": len(data), "records": a.value,
                                  "bytes_written": written, "read_engine_write_total_s": rows}), flush=True)
                for f in os.listdir(args.workdir):
                    if f.startswith("out_") and not os.path.isdir(os.path.join(args.workdir, f)):
                        os.remove(os.path.join(args.workdir, f))
    H.hpgv_run_set_output_compression(0)
    shutil.rmtree(args.workdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256, help="MB of text per kernel call")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--run-mb", type=int, default=512, help="MB of text of the whole-run file")
    ap.add_argument("--workdir", default="/tmp/hpgv_bench_bgzf")
    args = ap.parse_args()
    L = hpgv.load()
    ctx = C.c_void_p()
    assert L.hpgv_create(0, C.byref(ctx)) == 0
    for ns in (10000, 200):
        bench_kernel(args, L, ctx, ns)
    L.hpgv_destroy(ctx)
    if not args.kernel_only:
        bench_runs(args)


if __name__ == "__main__":
    main()
