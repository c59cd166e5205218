#!/usr/bin/env python3
"""The logistic regression's numbers (DESIGN.md "Logistic regression", k_logistic): hpgv_assoc_logistic_dev on resident
hpgv_synth_dev rows in the assoc layout, --samples cohort columns (half affected), --variants rows, for every C of --covars, with
standard normal covariates.  Kernel times are HIP events around the launch (option "profile"): the median, minimum and maximum of
--iters runs after --warmup.  Beside the times: variants per second, the Newton steps the rows took, and the achieved f64 FMA rate
by the definition's own count -- per observation and step p (p + 1) / 2 fma for H, p for u and p - 1 for eta (the p products
w x_i, the exp and the solve are not counted) -- against the vector pipe's 256 CUs x 4 SIMDs x 16 lanes x clock.  A spot check
refits the first rows with hpgv_logistic_fit on the host.  One JSON document on stdout and in --out."""
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


def classify(b):
    lo, hi = b & 15, b >> 4
    return np.where((lo == 15) | (hi == 15), 255, (lo != 0).astype(np.uint8) + (hi != 0)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--variants", type=int, default=4096)
    ap.add_argument("--covars", type=int, nargs="+", default=[0, 4, 10, 14])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-iter", type=int, default=25)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, V = a.samples, a.variants
    nA = N // 2
    cond = np.array([1] * nA + [0] * (N - nA), np.uint8)
    rng = np.random.default_rng(5)
    cov_all = rng.standard_normal((N, max(a.covars + [1])))
    e = hpgv.Engine(0)
    e.set_option("profile", 1)
    _, _, pitch = e.set_cohort(cond)
    segA = -(-nA // 16) * 16
    pos_of_col = np.concatenate([np.arange(nA), segA + np.arange(N - nA)])
    d_gt, d_out = e.alloc(V * pitch), e.alloc(V * 48)
    e.synth(hpgv.LAYOUT_ASSOC, 0, V, d_gt)
    e.sync()
    head = e.d2h(d_gt, (min(V, 4), pitch), np.uint8)[:, pos_of_col]
    peak = a.cus * 4 * 16 * a.clock_ghz * 1e9                     # f64 fma per second of the vector pipe at the nominal clock
    runs = []
    for C_ in a.covars:
        e.set_covariates(cov_all[:, :C_] if C_ else None)
        p = C_ + 2
        ts = []
        for r in range(a.warmup + a.iters):
            e.assoc_logistic_dev(d_gt, V, d_out, None, a.max_iter, a.tol)
            e.sync()
            if r >= a.warmup:
                ts.append(e.last_kernel_ms()[1])
        out = e.d2h(d_out, (V,), hpgv.LOGISTIC_RESULT)
        ok = True
        for r in range(len(head)):                               # the host fit of the first rows
            rec, _ = hpgv.logistic_fit(classify(head[r]), cond, cov_all[:, :C_] if C_ else None, a.max_iter, a.tol)
            same = rec["status"] == out[r]["status"] and rec["n_obs"] == out[r]["n_obs"]
            if same and rec["status"] == hpgv.LOGIT_OK:
                same = abs(rec["beta"] - out[r]["beta"]) <= 1e-10 * rec["se"] and abs(rec["se"] - out[r]["se"]) <= 1e-10 * rec["se"]
            ok = ok and bool(same)
        s = summary(ts)
        fma = float(np.sum(out["n_obs"].astype(np.float64) * out["iters"])) * (p * (p + 1) // 2 + p + p - 1)
        sec = s["ms_med"] * 1e-3
        s.update(covariates=C_, p=p, variants_per_s=round(V / sec, 1), rows_ok=int((out["status"] == hpgv.LOGIT_OK).sum()),
                 steps_mean=round(float(out["iters"].mean()), 3), fma_counted=fma, fma_per_s=round(fma / sec, 1),
                 vector_pipe_share_at_clock=round(fma / sec / peak, 4), covariate_bytes=C_ * pitch * 8, first_rows_equal_host_fit=ok)
        runs.append(s)
    e.close()
    doc = {"bench": "logistic", "samples": N, "variants": V, "pitch": pitch, "max_iter": a.max_iter, "tol": a.tol, "iters": a.iters,
           "warmup": a.warmup, "clock_ghz": a.clock_ghz, "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
