#!/usr/bin/env python3
"""The principal components' numbers (DESIGN.md "PCA"): k_pca_apply at --sizes (default 16 384 and 50 000) and L = 16 and 32 on a
resident matrix of one repeated f64 value -- the time, the achieved bytes/s against the 8 n^2 bytes of A and the FLOP/s of
2 n^2 L -- and hpgv_pca_dev at k = --k on a planted-structure matrix of --solve-n samples (the correlation of standardised
genotypes of four populations): sweeps, wall time, the residuals it reports.  Kernel times are HIP events around the launch
(option "profile"): median, minimum and maximum of --iters runs after --warmup.  With an ablation build (HPGV_LIB=
hpg-variant_amd/lib/ablation/libhpgv.so, tools/build_ablation.py) the lane-per-row v_fma_f64 form (option "pca_apply_vector") is
ALTERNATED with the shipped matrix-core form on the same buffers.  One JSON document on stdout and in --out."""
import argparse
import json
import os
import sys
import time
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
hpgv = import_module("hpg-variant_amd")
from bench_ibs import summary          # noqa: E402

FILL = 0x3F                            # every byte of A and Q: the f64 0x3F3F3F3F3F3F3F3F = 4.7e-4


def planted(n, m, groups, seed):
    """Z Z^T / m of standardised genotypes Z [n, m] of `groups` populations (allele frequencies clip(p + N(0, 0.25), 0.05, 0.95))"""
    rng = np.random.default_rng(seed)
    g = np.arange(n) % groups
    p = rng.uniform(0.1, 0.9, m)
    f = np.clip(p[None, :] + rng.normal(0.0, 0.25, (groups, m)), 0.05, 0.95)[g]
    Z = (rng.random((n, m)) < f).astype(np.float64) + (rng.random((n, m)) < f)
    Z -= Z.mean(axis=0)
    Z /= Z.std(axis=0) + 1e-12
    return Z @ Z.T / m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[16384, 50000])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--solve-n", type=int, default=8192)
    ap.add_argument("--solve-variants", type=int, default=4096)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    e = hpgv.Engine(0)
    e.set_option("profile", 1)
    try:
        e.set_option("pca_apply_vector", 1)
        e.set_option("pca_apply_vector", 0)
        forms = [("mfma", 0), ("vector", 1)]
    except hpgv.HpgvError:
        forms = [("mfma", 0)]                                       # the shipped library holds one form
    value = float(np.frombuffer(bytes([FILL] * 8), np.float64)[0])
    runs = []
    for n in a.sizes:
        lda = (n + 1) & ~1
        d_A = e.alloc(n * lda * 8)
        e.memset_dev(d_A, FILL, n * lda * 8)
        for L in (16, 32):
            d_Q, d_Y = e.alloc(n * L * 8), e.alloc(n * L * 8)
            e.memset_dev(d_Q, FILL, n * L * 8)
            ts = {name: [] for name, _ in forms}
            ok = {}
            for r in range(a.warmup + a.iters):
                for name, opt in forms:                             # alternated: the forms see the same clocks and the same cache state
                    if len(forms) > 1:
                        e.set_option("pca_apply_vector", opt)
                    e.pca_apply_dev(d_A, n, lda, d_Q, L, d_Y)
                    e.sync()
                    if r >= a.warmup:
                        ts[name].append(e.last_kernel_ms()[1])
                    elif r == 0:
                        y = e.d2h(d_Y, (n, L), np.float64)
                        ok[name] = bool(np.abs(y / (n * value * value) - 1.0).max() < 1e-12)
            if len(forms) > 1:
                e.set_option("pca_apply_vector", 0)
            for name, _ in forms:
                s = summary(ts[name])
                sec = s["ms_med"] * 1e-3
                s.update(form=name, n=n, L=L, lda=lda, workgroups=-(-n // 64), bytes_A=8 * n * n, bytes_per_s=round(8.0 * n * n / sec, 1),
                         flop_per_s=round(2.0 * n * n * L / sec, 1), product_is_n_a_q=ok[name])
                runs.append(s)
            e.free(d_Q)
            e.free(d_Y)
        e.free(d_A)
    # the solver on a matrix with structure
    n = a.solve_n
    t0 = time.time()
    A = planted(n, a.solve_variants, 4, 5)
    t_build = time.time() - t0
    lda = (n + 1) & ~1
    pad = np.zeros((n, lda))
    pad[:, :n] = A
    d_A = e.alloc(pad.nbytes)
    e.h2d(d_A, pad)
    t0 = time.time()
    out = e.pca_dev(d_A, n, lda, a.k, a.tol, 1000, 1)
    wall = time.time() - t0
    t0 = time.time()
    out2 = e.pca_dev(d_A, n, lda, a.k, a.tol, 1000, 1)
    wall2 = time.time() - t0
    e.free(d_A)
    X, val = out["vec"], out["eigval"]
    true_res = np.linalg.norm(A @ X - X * val, axis=0)
    solve = dict(n=n, variants=a.solve_variants, groups=4, k=a.k, L=hpgv.pca_block(a.k), tol=a.tol, sweeps=out["n_iter"], converged=out["converged"],
                 wall_s_first=round(wall, 4), wall_s_second=round(wall2, 4), ms_per_sweep=round(1e3 * wall2 / max(out["n_iter"], 1), 4),
                 eigenvalues=[round(float(v), 6) for v in val], resid_max=float(out["resid"].max()), resid_recomputed_max=float(true_res.max()),
                 second_call_identical=bool(np.array_equal(out["vec"], out2["vec"]) and np.array_equal(out["eigval"], out2["eigval"])),
                 host_matrix_build_s=round(t_build, 2))
    e.close()
    doc = {"bench": "pca", "iters": a.iters, "warmup": a.warmup, "forms": [f for f, _ in forms], "apply": runs, "solve": solve}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
