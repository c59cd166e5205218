#!/usr/bin/env python3
"""Wall time of hpgv_group_epi_rank: every member ranks its share, the top lists are handed over onto member 0 and merged.
Diagnostic tool.
  python tools/bench_group_epi_rank.py [--devices 0,0,0] [order] [V] [N] [k] [--top T] [--runs R]
Prints one JSON line: every run's wall time, their median and spread (the first call warms up and is not counted)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hpgv = importlib.import_module("hpg-variant_amd")

ap = argparse.ArgumentParser()
ap.add_argument("order", nargs="?", type=int, default=2)
ap.add_argument("V", nargs="?", type=int, default=2000)
ap.add_argument("N", nargs="?", type=int, default=1000)
ap.add_argument("K", nargs="?", type=int, default=5)
ap.add_argument("--devices", default="0,0,0")
ap.add_argument("--top", type=int, default=50)
ap.add_argument("--runs", type=int, default=5)
a = ap.parse_args()
rng = np.random.default_rng(1)
nA = nU = a.N // 2
data = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(a.V, nA + nU), p=[0.5, 0.35, 0.14, 0.01])
fold = np.empty(nA + nU, np.int32)
fold[rng.permutation(nA)] = np.arange(nA) % a.K
fold[nA + rng.permutation(nU)] = np.arange(nU) % a.K
devices = [int(d) for d in a.devices.split(",")]
g = hpgv.Engine(devices)
g.epi_set_dataset(data, nA, nU)
g.epi_set_folds(fold, a.K)
wall = []
for r in range(a.runs + 1):
    t0 = time.perf_counter()
    res = g.group_epi_rank(a.order, hpgv.EPI_TESTING, a.top)
    if r:
        wall.append((time.perf_counter() - t0) * 1e3)
print(json.dumps({"devices": devices, "order": a.order, "V": a.V, "samples": nA + nU, "folds": a.K, "top": a.top,
                  "wall_ms_runs": [round(t, 3) for t in wall], "wall_ms": round(statistics.median(wall), 3),
                  "wall_ms_min": round(min(wall), 3), "wall_ms_max": round(max(wall), 3), "scan_ms": round(res["scan_ms"], 3)}))
g.close()
