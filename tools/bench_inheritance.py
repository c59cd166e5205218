#!/usr/bin/env python3
"""The inheritance filters' numbers (DESIGN.md "Kernels", the inheritance scan):
  scan     hpgv_inheritance_scan_dev on --variants x --samples rows of HPGV_LAYOUT_ASSOC (half affected, half unaffected):
           kernel time (hipEvents around the launch, median of --iters), the rate (pitch + 32 bytes per row) / time as a share
           of the 8 TB/s HBM peak, and next to it the streaming-read probe over the same buffer (the ceiling)
  layout   hpgv_layout_dev(HPGV_LAYOUT_ASSOC) of the raw matrix the text path hands over (wall time around the launches,
           median of --iters): the pass the text path runs before the scan
  text     hpgv_filter_text on one --batch-lines batch of --samples samples, without a filter and with --inh-dom 0.5 (wall
           time, median of --iters)
One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hpgv = import_module("hpg-variant_amd")
HBM_PEAK = 8.0e12


def emit(d):
    print(json.dumps(d), flush=True)


def bench_scan(a, e):
    V, N = a.variants, a.samples
    cond = (np.arange(N) % 2).astype(np.uint8)
    _, _, pitch = e.set_cohort(cond)
    d_gt, d_c8 = e.alloc(V * pitch), e.alloc(V * 32)
    e.synth(hpgv.LAYOUT_ASSOC, 0, V, d_gt)
    e.sync()
    e.set_option("profile", 1)
    ts = []
    for r in range(a.iters + 2):
        e.inheritance_scan(d_gt, V, d_c8)
        e.sync()
        ms, _ = e.last_kernel_ms()
        if r >= 2:
            ts.append(ms)
    e.set_option("profile", 0)
    probe = e.read_probe(d_gt, V * pitch, 5)
    med = float(np.median(ts))
    rate = V * (pitch + 32) / (med * 1e-3)
    emit({"bench": "inheritance_scan", "variants": V, "samples": N, "pitch": pitch, "ms_med": round(med, 4), "ms_min": round(min(ts), 4),
          "GBps": round(rate / 1e9, 1), "frac_hbm_peak": round(rate / HBM_PEAK, 4),
          "read_probe_ms": round(probe, 4), "read_probe_frac": round(V * pitch / (probe * 1e-3) / HBM_PEAK, 4)})
    e.free(d_gt); e.free(d_c8)
    # the layout pass of the text path: raw rows (VCF order, n_samples rounded to 16) -> assoc rows
    raw_pitch = (N + 15) // 16 * 16
    Vl = min(V, a.layout_variants)
    d_raw, d_lay = e.alloc(Vl * raw_pitch), e.alloc(Vl * pitch)
    e.synth_raw(0, Vl, N, raw_pitch, d_raw)
    e.sync()
    ts = []
    for r in range(a.iters + 2):
        t0 = time.perf_counter()
        e.layout(hpgv.LAYOUT_ASSOC, d_raw, raw_pitch, Vl, d_lay)
        e.sync()
        if r >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(ts))
    rate = Vl * (raw_pitch + pitch) / (med * 1e-3)
    emit({"bench": "assoc_layout", "variants": Vl, "samples": N, "ms_med": round(med, 4), "GBps": round(rate / 1e9, 1),
          "frac_hbm_peak": round(rate / HBM_PEAK, 4)})
    e.free(d_raw); e.free(d_lay)


def bench_text(a, e):
    N, n = a.samples, a.batch_lines
    rng = np.random.default_rng(1)
    gts = np.array(["0/0", "0/1", "1/1", "./."])
    cond = rng.integers(0, 3, N).astype(np.uint8)
    e.set_stats_cohort(N)
    e.set_cohort(cond)
    body = ["\t".join(gts[rng.choice(4, N, p=[0.45, 0.35, 0.15, 0.05])]) for _ in range(64)]      # 64 distinct rows, cycled
    rows = ["1\t%d\trs%d\tA\tC\t50\tPASS\t.\tGT\t%s\n" % (100 + v, v, body[v % 64]) for v in range(n)]
    text = "".join(rows).encode()
    L = e.L
    L.hpgv_filter_text.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]
    L.hpgv_text_partition.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    buf = e.host_array(len(text) + 16)                        # page-locked, as the runners' batches are
    buf[:len(text)] = np.frombuffer(text, np.uint8)
    pbuf = C.cast(C.c_void_p(buf.ctypes.data), C.c_char_p)
    line_off, field_off, status = np.zeros(n + 1, np.uint64), np.zeros(10 * n, np.uint32), np.zeros(n, np.int32)
    for dom in (-1.0, 0.5):
        e.set_text_inheritance_filters(dom, -1.0)
        ts, kept = [], 0
        for r in range(a.iters + 2):
            nl = C.c_int()
            t0 = time.perf_counter()
            rc = L.hpgv_filter_text(e.h, pbuf, len(text), n, C.byref(nl), line_off.ctypes.data, field_off.ctypes.data, status.ctypes.data)
            dt = (time.perf_counter() - t0) * 1e3
            L.hpgv_text_partition(e.h, pbuf, None, 0, None, 0, None, None)
            assert rc == 0 and nl.value == n, L.hpgv_last_error(e.h)
            kept = int(((status & 0x100) == 0).sum())
            if r >= 2:
                ts.append(dt)
        med = float(np.median(ts))
        emit({"bench": "filter_text", "inh_dom": dom, "lines": n, "samples": N, "text_MB": round(len(text) / 1e6, 1),
              "ms_med": round(med, 3), "ms_min": round(min(ts), 3), "kept": kept, "GBps_text": round(len(text) / (med * 1e-3) / 1e9, 2)})
    e.set_text_inheritance_filters(-1.0, -1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=1_000_000)
    ap.add_argument("--samples", type=int, default=10_000)
    ap.add_argument("--layout-variants", type=int, default=200_000)
    ap.add_argument("--batch-lines", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    e = hpgv.Engine(0)
    try:
        bench_scan(a, e)
        bench_text(a, e)
    finally:
        e.close()


if __name__ == "__main__":
    main()
