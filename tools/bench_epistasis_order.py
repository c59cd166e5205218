#!/usr/bin/env python3
"""Throughput of the any-order MDR ranking (hpgv_epi_rank_order: the listed-combination kernels k_epi_combs and k_epi_combs_wide,
one lane per cell of the 3^order table): all C(V, order) combinations x N samples x k folds.  Diagnostic tool.
  python tools/bench_epistasis_order.py [order] [V] [N] [k] [--runs R] [--wide W | --wide 0,2]
--wide W sets option "epi_wide" (0: the packed kernel's limits, 1: the wide kernel where the shape needs it, 2: the wide kernel
everywhere); a list alternates its values run by run on one engine (an A/B of the two kernels on a shape both take).  Without
--wide the option is left alone.  Per variant: every run's scan time, the median and the spread (min .. max)."""
import argparse
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hpgv = importlib.import_module("hpg-variant_amd")

ap = argparse.ArgumentParser()
ap.add_argument("order", nargs="?", type=int, default=4)
ap.add_argument("V", nargs="?", type=int, default=96)
ap.add_argument("N", nargs="?", type=int, default=10000)
ap.add_argument("K", nargs="?", type=int, default=10)
ap.add_argument("--runs", type=int, default=2)
ap.add_argument("--wide", default=None)
a = ap.parse_args()
order, V, N, K = a.order, a.V, a.N, a.K
variants = [None] if a.wide is None else [int(w) for w in a.wide.split(",")]
rng = np.random.default_rng(1)
nA = nU = N // 2
data = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(V, nA + nU), p=[0.5, 0.35, 0.14, 0.01])
fold = np.empty(nA + nU, np.int32)
fold[rng.permutation(nA)] = np.arange(nA) % K
fold[nA + rng.permutation(nU)] = np.arange(nU) % K
e = hpgv.Engine(0)
if variants[0] is not None:
    e.set_option("epi_wide", max(variants))                          # the layout is built once, under the widest setting asked for
e.epi_set_dataset(data, nA, nU)
e.epi_set_folds(fold, K)
combs = math.comb(V, order)
runs = {w: [] for w in variants}
kernel = {}
for r in range(a.runs + 1):                                          # (the first round warms up)
    for w in variants:
        if w is not None:
            e.set_option("epi_wide", w)
        t0 = time.perf_counter()
        res = e.epi_rank_order(order, hpgv.EPI_TESTING, 10)
        if r:
            runs[w].append((time.perf_counter() - t0, res["scan_ms"]))
        kernel[w] = e.epi_last_rank_info()["kernel_name"]
for w in variants:
    scan = sorted(ms for _, ms in runs[w])
    med = statistics.median(scan)
    print(json.dumps({"order": order, "V": V, "samples": N, "folds": K, "epi_wide": w, "kernel": kernel[w], "combinations": combs,
                      "wall_s": round(min(t for t, _ in runs[w]), 4), "scan_ms_runs": [round(ms, 3) for _, ms in runs[w]],
                      "scan_ms": round(med, 3), "scan_ms_min": round(scan[0], 3), "scan_ms_max": round(scan[-1], 3),
                      "combinations_per_s": combs / (med * 1e-3), "cells_per_combination": 3 ** order,
                      "cell_samples_per_s": combs * 3 ** order * N / (med * 1e-3)}))
e.close()
