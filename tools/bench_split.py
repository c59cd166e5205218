#!/usr/bin/env python3
"""The split tool's numbers (DESIGN.md "Partition of lines"):
  kernel   hpgv_lines_multisplit_dev on 256 MB of lines of 10 000 samples (~40 KB) and of 200 samples (~800 B), with 2 buckets
           (every other line), 25 buckets in sorted runs and 255 buckets of random ids; hpgv_lines_partition_dev on the same
           text as the comparison.  Wall time per call over --iters calls, split into the offset stage (the same call with
           every id >= n_buckets: nothing copied) and the copy (the rest); rates as (bytes read + written) / time against the
           8 TB/s HBM peak.
  run      hpgv_run_split by chromosome (24 contigs in runs) and by coverage (4 intervals) on a 10 000-sample file, plain and
           bgzip, next to hpgv_host_copy_lines on the same file (the reader alone writing every line).  Wall and stage times,
           and the host time of the key loop (HPGV_RUN_TRACE's "split keys" line, summed over the engine threads).
One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import time
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
hpgv = import_module("hpg-variant_amd")
from bench_filter import HBM_PEAK, bgzf, lines_of  # noqa: E402


def timed(L, ctx, call, iters):
    for _ in range(3):
        assert call() == 0, L.hpgv_last_error(ctx)
    assert L.hpgv_stream_sync(ctx, None) == 0
    t0 = time.perf_counter()
    for _ in range(iters):
        call()
    assert L.hpgv_stream_sync(ctx, None) == 0
    return (time.perf_counter() - t0) / iters


def bench_kernel(args, L, ctx, n_samples):
    rng = np.random.default_rng(n_samples)
    text, off = lines_of(n_samples, args.mb << 20, rng)
    n = len(off) - 1
    vp = C.c_void_p
    bufs = []

    def alloc(b):
        p = vp()
        assert L.hpgv_dev_alloc(ctx, b, C.byref(p)) == 0
        bufs.append(p)
        return p.value

    d_text, d_off, d_ids, d_none = alloc(text.nbytes + 16), alloc(off.nbytes), alloc(n), alloc(n)
    d_out, d_kept, d_boff = alloc(text.nbytes + 16), alloc(8), alloc(8 * 257)
    d_scr = alloc(max(L.hpgv_lines_multisplit_scratch_bytes(n, 256), L.hpgv_lines_partition_scratch_bytes(n)))
    for d, a in ((d_text, text), (d_off, off)):
        assert L.hpgv_memcpy_h2d(ctx, d, a.ctypes.data, a.nbytes, None) == 0
    none = np.full(n, 255, np.uint8)
    assert L.hpgv_memcpy_h2d(ctx, d_none, none.ctypes.data, n, None) == 0
    moved = 2.0 * text.nbytes
    keep = (np.arange(n) % 2).astype(np.uint8)
    assert L.hpgv_memcpy_h2d(ctx, d_ids, keep.ctypes.data, n, None) == 0
    part = timed(L, ctx, lambda: L.hpgv_lines_partition_dev(ctx, d_text, d_off, n, d_ids, d_out + 3, d_kept, d_scr, None), args.iters)
    print(json.dumps({"what": "partition_kernel", "samples": n_samples, "lines": n, "bytes": int(text.nbytes),
                      "ms_per_call": round(part * 1e3, 4), "share_of_hbm_peak": round(moved / part / HBM_PEAK, 3)}), flush=True)
    cases = {2: (1 - keep).astype(np.uint8), 25: np.sort(rng.integers(0, 25, n)).astype(np.uint8),
             255: rng.integers(0, 255, n).astype(np.uint8)}
    for nb, ids in cases.items():
        assert L.hpgv_memcpy_h2d(ctx, d_ids, ids.ctypes.data, n, None) == 0
        full = timed(L, ctx, lambda: L.hpgv_lines_multisplit_dev(ctx, d_text, d_off, n, d_ids, nb, d_out + 3, d_boff, d_scr, None), args.iters)
        got = np.empty(text.nbytes, np.uint8)
        assert L.hpgv_memcpy_d2h(ctx, got.ctypes.data, d_out + 3, got.nbytes, None) == 0
        order = np.argsort(ids, kind="stable")
        exp = np.concatenate([text[int(off[i]):int(off[i + 1])] for i in order])
        assert np.array_equal(got, exp)
        offs = timed(L, ctx, lambda: L.hpgv_lines_multisplit_dev(ctx, d_text, d_off, n, d_none, nb, d_out + 3, d_boff, d_scr, None), args.iters)
        copy = max(full - offs, 1e-9)
        print(json.dumps({"what": "multisplit_kernel", "samples": n_samples, "lines": n, "bytes": int(text.nbytes), "buckets": nb,
                          "ids": "every other line" if nb == 2 else "sorted runs" if nb == 25 else "random",
                          "ms_per_call": round(full * 1e3, 4), "offset_stage_ms": round(offs * 1e3, 4), "copy_ms": round(copy * 1e3, 4),
                          "copy_share_of_hbm_peak": round(moved / copy / HBM_PEAK, 3), "call_share_of_hbm_peak": round(moved / full / HBM_PEAK, 3),
                          "ratio_to_partition": round(full / part, 3)}), flush=True)
    for p in bufs:
        L.hpgv_dev_free(ctx, p)


def bench_run(args, n_samples):
    H = C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)
    H.hpgv_run_split.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_long), C.c_int, C.c_size_t,
                                 C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]
    H.hpgv_host_copy_lines.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_long)]
    H.hpgv_host_last_error.restype = C.c_char_p
    os.makedirs(args.workdir, exist_ok=True)
    rec = "\t0/1" * n_samples + "\n"
    n_rec = max(2, (args.run_mb << 20) // (len(rec) + 48))
    hdr = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + "".join("\ts%d" % j for j in range(n_samples)) + "\n"
    contigs = ["chr%d" % k for k in range(1, 23)] + ["chrX", "chrY"]
    body = "".join("%s\t%d\trs%d\tA\tC\t50\tPASS\tDP=%d;AF=0.5\tGT%s" % (contigs[v * 24 // n_rec], 100 + v, v, (v * 37) % 120, rec)
                   for v in range(n_rec))
    data = (hdr + body).encode()
    paths = {"plain": os.path.join(args.workdir, "f.vcf"), "bgzip": os.path.join(args.workdir, "f.vcf.gz")}
    with open(paths["plain"], "wb") as f:
        f.write(data)
    with open(paths["bgzip"], "wb") as f:
        f.write(bgzf(data))
    del data, body
    t = (C.c_double * 6)()
    iv = (C.c_long * 4)(10, 30, 60, 90)
    out = os.path.join(args.workdir, "out")
    for kind, path in paths.items():
        for crit, name in ((1, "chromosome"), (2, "coverage")):
            for rep in range(2):                                   # the first run warms the page cache and the engine
                shutil.rmtree(out, ignore_errors=True)
                a, nf, ns = C.c_long(0), C.c_long(0), C.c_long(0)
                err = os.path.join(args.workdir, "trace")
                saved = os.dup(2)
                fd = os.open(err, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                os.dup2(fd, 2)
                os.close(fd)
                t0 = time.perf_counter()
                rc = H.hpgv_run_split(path.encode(), out.encode(), crit, iv, 4, 1 << 26, C.byref(a), C.byref(nf), C.byref(ns))
                wall = time.perf_counter() - t0
                os.dup2(saved, 2)
                os.close(saved)
                assert rc == 0, H.hpgv_host_last_error()
                keys = [float(l.split()[4]) for l in open(err) if l.startswith("hpgv run: split keys")]
                H.hpgv_host_last_run_times(t)
                nb = C.c_long(0)
                t0 = time.perf_counter()
                rc = H.hpgv_host_copy_lines(path.encode(), os.path.join(args.workdir, "copy").encode(), 1 << 26, 1, C.byref(nb))
                copy = time.perf_counter() - t0
                assert rc == 0
            print(json.dumps({"what": "split_run", "criterion": name, "input": kind, "samples": n_samples, "records": a.value,
                              "files": nf.value, "text_bytes": os.path.getsize(paths["plain"]), "wall_s": round(wall, 4),
                              "stages_s": {"read": round(t[0], 4), "engine": round(t[1], 4), "write": round(t[2], 4), "total": round(t[4], 4),
                                           "host_keys": round(keys[0], 4) if keys else None},
                              "batches": int(t[5]), "copy_lines_s": round(copy, 4), "ratio_to_copy_lines": round(wall / copy, 3)}), flush=True)
    shutil.rmtree(args.workdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256, help="MB of lines per kernel call")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--run-mb", type=int, default=512, help="MB of text of the whole-run file")
    ap.add_argument("--workdir", default="/tmp/hpgv_bench_split")
    args = ap.parse_args()
    os.environ["HPGV_RUN_TRACE"] = "1"                             # the runs' stage lines (read when a run starts)
    L = hpgv.load()
    L.hpgv_lines_partition_scratch_bytes.argtypes = [C.c_int]
    L.hpgv_lines_partition_scratch_bytes.restype = C.c_size_t
    L.hpgv_lines_partition_dev.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 5
    L.hpgv_lines_multisplit_scratch_bytes.argtypes = [C.c_int, C.c_int]
    L.hpgv_lines_multisplit_scratch_bytes.restype = C.c_size_t
    L.hpgv_lines_multisplit_dev.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4
    ctx = C.c_void_p()
    assert L.hpgv_create(0, C.byref(ctx)) == 0
    for ns in (10000, 200):
        bench_kernel(args, L, ctx, ns)
    L.hpgv_destroy(ctx)
    if not args.kernel_only:
        bench_run(args, 10000)


if __name__ == "__main__":
    main()
