#!/usr/bin/env python3
"""Allele scoring's numbers (DESIGN.md "Score", k_score_cols): hpgv_score_cols_dev on a resident matrix at the shapes samples x
variants of --shapes (default 10 000 x 65 536, many column tiles, and 200 x 4 000 000, four tiles cut into row ranges), for
--scores weight columns (default 1, 4, 8, 24), with and without --missing (default 2 %) missing calls, and in the same run
hpgv_read_probe over the same buffer: what one read of the matrix costs.  Kernel times are HIP events around the launch (option
"profile"): the median, minimum and maximum of --iters runs after --warmup, the sums zeroed before each.  The rows' tables are made
once per case, by hpgv_ibs_class_counts_dev and hpgv_score_table_dev, and are not part of the time.  The matrix is a block of 4 096
random rows repeated: the kernels' work does not depend on the values.  One JSON document on stdout and in --out."""
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

BLOCK = 4096


def matrix(n_cols, n_variants, pitch, p_missing, seed):
    """[n_variants, pitch] HPGV8: 0/0, 0/1, 1/1 by a frequency per row, p_missing of ./., pads 0xFF; BLOCK rows repeated"""
    rng = np.random.default_rng(seed)
    rows = min(BLOCK, n_variants)
    p = rng.uniform(0.05, 0.5, rows)[:, None]
    a, b = rng.random((rows, n_cols)) < p, rng.random((rows, n_cols)) < p
    codes = (a.astype(np.uint8) << 4) | b.astype(np.uint8)
    codes[rng.random((rows, n_cols)) < p_missing] = 0xFF
    blk = np.full((rows, pitch), 0xFF, np.uint8)
    blk[:, :n_cols] = codes
    return np.ascontiguousarray(np.tile(blk, (-(-n_variants // rows), 1))[:n_variants])


def golden(codes, w, s, flags, impute):
    """(acc int64 [n_scores + 2, cols], const [n_scores + 1]) of a code matrix, the table by hpgv_score_table"""
    hi, lo = codes >> 4, codes & 15
    v = (hi != 15) & (lo != 15)
    g = np.where(v, (hi != 0).astype(np.int64) + (lo != 0), 0)
    c3 = np.stack([(v & (g == c)).sum(axis=1) for c in range(3)], axis=1)
    used, lim, c = hpgv.score_table(c3, w, s, flags, impute)
    place = np.array([1, 256, 65536, 1 << 24], np.int64)
    qg, qm = (lim[:, :, :4].astype(np.int64) * place).sum(axis=-1), (lim[:, :, 4:].astype(np.int64) * place).sum(axis=-1)
    G, V, M = g * used[:, None], (v & used[:, None]).astype(np.int64), (~v & used[:, None]).astype(np.int64)
    return np.concatenate([qg.T @ G + qm.T @ M, V.sum(axis=0)[None], G.sum(axis=0)[None]]), np.concatenate([c.sum(axis=0), [used.sum()]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["10000x65536", "200x4000000"], help="samples x variants")
    ap.add_argument("--scores", nargs="+", type=int, default=[1, 4, 8, 24])
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    e = hpgv.Engine(0)
    e.set_option("profile", 1)
    runs = []
    for shape in a.shapes:
        N, V = (int(x) for x in shape.split("x"))
        pitch, tab_pitch = -(-N // 16) * 16, -(-V // 64) * 64
        K = max(a.scores)
        d_gt, d_c4, d_skip, d_fl = e.alloc(V * pitch), e.alloc(V * 16), e.alloc(V + 16), e.alloc(V + 16)
        d_w, d_tab, d_acc, d_const = e.alloc(V * K * 8), e.alloc(tab_pitch * 8 * K), e.alloc((K + 2) * N * 8), e.alloc((K + 1) * 8)
        rng = np.random.default_rng(7)
        flags = np.where(rng.random(V) < 1 / 3, 2, 0).astype(np.uint8)
        e.h2d(d_fl, flags)
        for p_missing in (0.0, a.missing):
            gt = matrix(N, V, pitch, p_missing, 11)
            e.h2d(d_gt, gt)
            probe_ms = e.read_probe(d_gt, V * pitch, iters=a.iters)
            for ns in a.scores:
                w = rng.standard_normal((V, ns))
                s = np.array([hpgv.score_frac_bits(np.abs(w[:, k]).max()) for k in range(ns)], np.int32)
                e.h2d(d_w, w)
                e.memset_dev(d_skip, 0, V)
                e.memset_dev(d_const, 0, (ns + 1) * 8)
                e.ibs_class_counts_dev(d_gt, pitch, V, N, d_c4, d_skip=d_skip)
                e.score_table_dev(d_c4, V, d_w, d_fl, s, 1, d_skip, d_tab, tab_pitch, d_const)
                e.sync()
                ts = []
                for r in range(a.warmup + a.iters):
                    e.memset_dev(d_acc, 0, (ns + 2) * N * 8)
                    e.score_cols_dev(d_gt, pitch, V, N, d_tab, tab_pitch, ns, d_acc, N, d_skip=d_skip)
                    e.sync()
                    if r >= a.warmup:
                        ts.append(e.last_kernel_ms()[1])
                # a spot check of what was timed: the first 48 columns over the first 3 000 rows, calls of their own, against numpy
                # (the table there is of the 48 columns' own class counts)
                nc, nr = min(N, 48), min(V, 3000)
                e.memset_dev(d_acc, 0, (ns + 2) * N * 8)
                e.memset_dev(d_const, 0, (ns + 1) * 8)
                e.memset_dev(d_skip, 0, nr)
                e.ibs_class_counts_dev(d_gt, pitch, nr, nc, d_c4, d_skip=d_skip)
                e.score_table_dev(d_c4, nr, d_w, d_fl, s, 1, d_skip, d_tab, tab_pitch, d_const)
                e.score_cols_dev(d_gt, pitch, nr, nc, d_tab, tab_pitch, ns, d_acc, N, d_skip=d_skip)
                e.sync()
                exp_acc, exp_const = golden(gt[:nr, :nc], w[:nr], s, flags[:nr], 1)
                ok = bool(np.array_equal(e.d2h(d_acc, (ns + 2, N), np.int64)[:, :nc], exp_acc) and exp_acc[:ns].any() and
                          np.array_equal(e.d2h(d_const, (ns + 1,), np.int64), exp_const))
                t = summary(ts)
                sec = t["ms_med"] * 1e-3
                rows = hpgv.score_plan_rows(V, N, ns, a.cus)
                t.update(rows_per_s=round(V / sec, 1), matrix_bytes_per_s=round(V * pitch / sec, 1), read_probe_ms=round(probe_ms, 4),
                         read_probe_bytes_per_s=round(V * pitch / (probe_ms * 1e-3), 1), ratio_to_read_probe=round(probe_ms / t["ms_med"], 4),
                         rows_per_range=rows, row_ranges=-(-V // rows), workgroups=-(-V // rows) * -(-N // 64))
                runs.append(dict(samples=N, variants=V, pitch=pitch, scores=ns, missing=p_missing, k_score_cols=t, sums_equal_numpy_on_first_columns=ok))
        for d in (d_gt, d_c4, d_skip, d_fl, d_w, d_tab, d_acc, d_const):
            e.free(d)
    e.close()
    doc = {"bench": "score_cols", "iters": a.iters, "warmup": a.warmup, "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
