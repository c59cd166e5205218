#!/usr/bin/env python3
"""The family-flip kernel's numbers (DESIGN.md "Kernels", k_tdt_perm) with k_assoc_perm beside it as the yardstick, both on a
synthetic cohort (hpgv_synth_dev) of --variants rows and K = --trios: hpgv_tdt_perm_dev over --trios one-child families
(3 x K sample columns) and hpgv_assoc_perm_dev over K sample columns, --perms permutations each.  Per kernel: the launch time
(HIP events around the launch, median of --iters after --warmup launches of the same shape), the time per (variant,
permutation, k), the number of v_mfma_i32_16x16x64_i8 the launch issues (16-row tiles x passes x k-steps x MFMAs per k-step: 8
for the one signed plane of the TDT, 16 for the two planes of the label form) and the share of the matrix pipes' time they
account for at 16 cycles per instruction on --cus x 4 SIMDs at --ghz.  Results as one JSON document on stdout and in --out."""
import argparse
import json
import os
import sys
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hpgv = import_module("hpg-variant_amd")
TILE_P, MFMA_CYCLES = 128, 16


def timed(launch, e, a):
    ts = []
    for r in range(a.warmup + a.iters):
        launch()
        e.sync()
        if r >= a.warmup:
            ts.append(e.last_kernel_ms()[1])
    return ts


def report(name, ts, V, K, kpitch, P, planes, a):
    med = float(np.median(ts))
    mfmas = -(-V // 16) * -(-P // TILE_P) * -(-(kpitch // 16) // 4) * (TILE_P // 16) * planes
    return {"kernel": name, "k": K, "k_pitch": kpitch, "ms_med": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
            "fs_per_variant_permutation_k": round(med * 1e-3 / (V * P * K) * 1e15, 3), "mfma_instructions": mfmas,
            "matrix_pipe_share": round(mfmas * MFMA_CYCLES / (a.cus * 4 * a.ghz * 1e9 * med * 1e-3), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=100000)
    ap.add_argument("--trios", type=int, default=5000)
    ap.add_argument("--perms", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    V, K, P = a.variants, a.trios, a.perms
    runs = []

    e = hpgv.Engine(0)
    k = np.arange(K)
    n_fast, n_slow, pitch = e.set_families(3 * K, 3 * k, 3 * k + 1, np.arange(K + 1), 3 * k + 2, (k % 2).astype(np.uint8))
    assert (n_fast, n_slow) == (K, 0)
    d_gt, d_tu, d_nge, d_max = e.alloc(V * pitch), e.alloc(V * 8), e.alloc(V * 4), e.alloc(P * 8)
    e.synth(hpgv.LAYOUT_TDT, 0, V, d_gt)
    e.tdt_scan(d_gt, V, d_tu)
    e.sync()
    e.set_tdt_flips(hpgv.perm_flips_shuffle(K, P, a.seed))
    e.set_option("profile", 1)
    ts = timed(lambda: e.tdt_perm_dev(d_gt, V, d_tu, d_nge, d_max), e, a)
    bmax = e.d2h(d_max, (P,), np.float64)
    runs.append(dict(report("k_tdt_perm", ts, V, K, -(-K // 16) * 16, P, 1, a), row_bytes=pitch, batch_max_mean=float(bmax.mean())))
    e.close()

    e = hpgv.Engine(0)
    cond = (np.arange(K) % 2).astype(np.uint8)
    _, _, pitch = e.set_cohort(cond)
    d_gt, d_counts, d_nge, d_max = e.alloc(V * pitch), e.alloc(V * 16), e.alloc(V * 4), e.alloc(P * 8)
    e.synth(hpgv.LAYOUT_ASSOC, 0, V, d_gt)
    e.assoc_scan(d_gt, V, d_counts)
    e.sync()
    e.set_perm_labels(hpgv.perm_labels_shuffle(cond, P, a.seed))
    e.set_option("profile", 1)
    ts = timed(lambda: e.assoc_perm_dev(d_gt, V, d_counts, d_nge, d_max), e, a)
    bmax = e.d2h(d_max, (P,), np.float64)
    runs.append(dict(report("k_assoc_perm", ts, V, K, pitch, P, 2, a), row_bytes=pitch, batch_max_mean=float(bmax.mean())))
    e.close()

    doc = {"bench": "tdt_perm", "variants": V, "permutations": P, "iters": a.iters, "warmup": a.warmup,
           "matrix_pipes": {"cus": a.cus, "simds_per_cu": 4, "ghz": a.ghz, "cycles_per_mfma": MFMA_CYCLES}, "runs": runs,
           "tdt_over_assoc_per_variant_permutation_k": round(runs[0]["ms_med"] / runs[1]["ms_med"], 4)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
