#!/usr/bin/env python3
"""The linear regression's numbers (DESIGN.md "Linear regression", k_linear): hpgv_assoc_linear_dev on resident hpgv_synth_dev rows
in the assoc layout, --samples cohort columns, --variants rows, for every C of --covars with standard normal covariates and a
standard normal trait, and for every missing rate of --missing (the synthetic rows' own missing calls are replaced: none, or that
share of the cohort positions at random).  Kernel times are HIP events around the launch (option "profile"): the median, minimum
and maximum of --iters runs after --warmup.  Beside the times: variants per second, the genotype bytes per second, and the f64
matrix-core rate by the kernel's own count -- 16 fma per position of a row, pads included -- against 256 CUs x 4 SIMDs x 16 fma
per clock.  A spot check refits the first rows with hpgv_linear_fit on the host.  One JSON document on stdout and in --out."""
import argparse
import json
import os
import sys
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
hpgv = import_module("hpg-variant_amd")
from bench_ibs import summary          # noqa: E402
from bench_logistic import classify    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--variants", type=int, default=4096)
    ap.add_argument("--covars", type=int, nargs="+", default=[0, 4, 10, 14])
    ap.add_argument("--missing", type=float, nargs="+", default=[0.0, 0.02])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, V = a.samples, a.variants
    nA = N // 2
    cond = np.array([1] * nA + [0] * (N - nA), np.uint8)
    rng = np.random.default_rng(5)
    cov_all = rng.standard_normal((N, max(a.covars + [1])))
    y = rng.standard_normal(N)
    e = hpgv.Engine(0)
    e.set_option("profile", 1)
    _, _, pitch = e.set_cohort(cond)
    segA = -(-nA // 16) * 16
    pos_of_col = np.concatenate([np.arange(nA), segA + np.arange(N - nA)])
    d_gt, d_out = e.alloc(V * pitch), e.alloc(V * 48)
    e.synth(hpgv.LAYOUT_ASSOC, 0, V, d_gt)
    e.sync()
    base = e.d2h(d_gt, (V, pitch), np.uint8)
    cohort = base[:, pos_of_col]
    cohort[classify(cohort) == 255] = 0x00
    peak = a.cus * 4 * 16 * a.clock_ghz * 1e9                     # f64 fma per second of the matrix cores at the nominal clock
    steps = -(-pitch // 64) * 64                                  # positions an MFMA pass walks per row
    runs = []
    for miss in a.missing:
        gt = base.copy()
        col = cohort.copy()
        if miss > 0:
            col[rng.random(col.shape) < miss] = 0xFF
        gt[:, pos_of_col] = col
        e.h2d(d_gt, gt)
        e.sync()
        for C_ in a.covars:
            e.set_covariates(cov_all[:, :C_] if C_ else None)
            e.set_phenotype(y)
            ts = []
            for r in range(a.warmup + a.iters):
                e.assoc_linear_dev(d_gt, V, d_out, None)
                e.sync()
                if r >= a.warmup:
                    ts.append(e.last_kernel_ms()[1])
            out = e.d2h(d_out, (V,), hpgv.LINEAR_RESULT)
            ok = True
            for r in range(min(V, 4)):                           # the host fit of the first rows
                rec, _ = hpgv.linear_fit(classify(col[r]), y, cov_all[:, :C_] if C_ else None)
                same = rec["status"] == out[r]["status"] and rec["n_obs"] == out[r]["n_obs"]
                if same and rec["status"] == hpgv.LINEAR_OK:
                    same = abs(rec["beta"] - out[r]["beta"]) <= 1e-10 * rec["se"] and abs(rec["se"] - out[r]["se"]) <= 1e-10 * rec["se"]
                ok = ok and bool(same)
            s = summary(ts)
            sec = s["ms_med"] * 1e-3
            fma = float(V) * steps * 16
            s.update(covariates=C_, p=C_ + 2, missing=miss, variants_per_s=round(V / sec, 1), rows_ok=int((out["status"] == hpgv.LINEAR_OK).sum()),
                     genotype_bytes_per_s=round(V * pitch / sec, 1), fma_counted=fma, fma_per_s=round(fma / sec, 1),
                     matrix_core_share_at_clock=round(fma / sec / peak, 4), image_bytes=steps * 128, first_rows_equal_host_fit=ok)
            runs.append(s)
    e.close()
    doc = {"bench": "linear", "samples": N, "variants": V, "pitch": pitch, "iters": a.iters, "warmup": a.warmup, "clock_ghz": a.clock_ghz, "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
