#!/usr/bin/env python3
"""The numbers of the linear statistic's permutations (DESIGN.md "Linear regression", k_linear_perm_rows and k_linear_perm):
hpgv_assoc_linear_perm_dev on resident hpgv_synth_dev rows in the assoc layout, for every shape of --shapes (samples x variants),
--perms permutations of hpgv_perm_order_shuffle, every C of --covars and every missing rate of --missing (the synthetic rows' own
missing calls are replaced: none, or that share of the cohort positions at random).  Kernel times are HIP events around the two
launches (option "profile"): the median, minimum and maximum of --iters runs after --warmup.  Beside each time, on the same matrix:
hpgv_assoc_linear_dev (the regression alone), hpgv_assoc_trend_perm_dev at the same shape with as many label rows (the i8 permutation
kernel), and the time that 2 planes x 2 flop x samples x variants x permutations would take at the f64 matrix-core rate that
hpgv_mfma_f64_probe measures in the same process.  A spot check holds the first rows against hpgv_linear_perm_fit.  One JSON document
on stdout and in --out."""
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


def timed(e, call, a, which=1):
    ts = []
    for r in range(a.warmup + a.iters):
        call()
        e.sync()
        if r >= a.warmup:
            ts.append(e.last_kernel_ms()[which])
    return summary(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["10000x4096", "200x65536"])
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--covars", type=int, nargs="+", default=[0, 14])
    ap.add_argument("--missing", type=float, nargs="+", default=[0.0, 0.02])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P = a.perms
    e = hpgv.Engine(0)
    probe_ms, probe_flop = e.mfma_f64_probe(4096, 5)
    rate = probe_flop / (probe_ms * 1e-3)
    e.set_option("profile", 1)
    runs = []
    for shape in a.shapes:
        N, V = (int(x) for x in shape.split("x"))
        nA = N // 2
        cond = np.array([1] * nA + [0] * (N - nA), np.uint8)
        rng = np.random.default_rng(5)
        cov_all = rng.standard_normal((N, max(a.covars + [1])))
        y = rng.standard_normal(N)
        _, _, pitch = e.set_cohort(cond)
        segA = -(-nA // 16) * 16
        pos_of_col = np.concatenate([np.arange(nA), segA + np.arange(N - nA)])
        bufs = [e.alloc(n) for n in (V * pitch, V * 48, V * 8, V * 4, P * 8, V * 32)]
        d_gt, d_out, d_t, d_ge, d_max, d_c8 = bufs
        e.synth(hpgv.LAYOUT_ASSOC, 0, V, d_gt)
        e.sync()
        base = e.d2h(d_gt, (V, pitch), np.uint8)
        cohort = base[:, pos_of_col]
        cohort[classify(cohort) == 255] = 0x00
        order = hpgv.perm_order_shuffle(cond, P, a.seed)
        e.set_perm_labels(hpgv.perm_labels_shuffle(cond, P, a.seed))
        flop = 2.0 * 2.0 * N * V * P
        for miss in a.missing:
            gt = base.copy()
            col = cohort.copy()
            if miss > 0:
                col[rng.random(col.shape) < miss] = 0xFF
            gt[:, pos_of_col] = col
            e.h2d(d_gt, gt)
            e.sync()
            e.assoc_model_scan(d_gt, V, d_c8)
            trend = timed(e, lambda: e.assoc_trend_perm_dev(d_gt, V, d_c8, d_ge, d_max), a)
            for C_ in a.covars:
                cv = cov_all[:, :C_] if C_ else None
                e.set_covariates(cv)
                e.set_phenotype(y)
                linear = timed(e, lambda: e.assoc_linear_dev(d_gt, V, d_out, None), a)
                e.set_linear_perms(order)
                s = timed(e, lambda: e.assoc_linear_perm_dev(d_gt, V, d_t, d_ge, d_max), a)
                t_obs, n_ge = e.d2h(d_t, (V,), np.float64), e.d2h(d_ge, (V,), np.int32)
                ok = True
                for r in range(min(V, 3)):                        # the host fit of the first rows
                    want, tp = hpgv.linear_perm_fit(classify(col[r]), y, cv, order)
                    ok = ok and (np.isnan(want) == np.isnan(t_obs[r])) and (np.isnan(want) or abs(want - t_obs[r]) <= 1e-9 * max(1.0, abs(want)))
                    ok = ok and (np.isnan(want) or abs(int((np.abs(tp) >= abs(want)).sum()) - int(n_ge[r])) <= 1)
                sec = s["ms_med"] * 1e-3
                s.update(samples=N, variants=V, pitch=pitch, permutations=P, covariates=C_, missing=miss, flop=flop, flop_per_s=round(flop / sec, 1),
                         share_of_probe_rate=round(flop / sec / rate, 4), ms_at_probe_rate=round(flop / rate * 1e3, 4),
                         linear_dev_ms_med=linear["ms_med"], trend_perm_dev_ms_med=trend["ms_med"], rows_taking_part=int((~np.isnan(t_obs)).sum()),
                         image_bytes=(1 + -(-P // 16)) * (-(-pitch // 64) * 64) * 128, first_rows_equal_host_fit=bool(ok))
                runs.append(s)
        e.set_linear_perms(None)
        for b in bufs:
            e.free(b)
    e.close()
    doc = {"bench": "linear_perm", "iters": a.iters, "warmup": a.warmup,
           "mfma_f64_probe": {"ms": round(probe_ms, 4), "flop": probe_flop, "flop_per_s": round(rate, 1)}, "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
