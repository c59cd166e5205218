#!/usr/bin/env python3
"""The relationship matrix's numbers beside the IBS counts' (DESIGN.md "GRM", k_grm_pairs against k_ibs_pairs): hpgv_grm_pairs_dev
and hpgv_ibs_pairs_dev ALTERNATED on the same resident hpgv_synth_raw_dev matrix at the shapes samples x variants of --shapes
(default 10 000 x 100 000, many tile pairs, and 200 x 1 000 000, ten tile pairs cut into row ranges).  Kernel times are HIP events
around the launch (option "profile"): the median, minimum and maximum of --iters runs after --warmup, the output buffer zeroed
before each.  The rows' tables are made once, by hpgv_ibs_class_counts_dev and hpgv_grm_table_dev at --frac-bits / --min-maf, and
are not part of the time.  Beside the times: their ratio, and the matrix-pipe share of each by the kernels' own rules (tools/
bench_ibs.py's `work`; 5 MFMAs per computed block and k-step for the GRM, 4 for IBS).  One JSON document on stdout and in --out."""
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
from bench_ibs import MFMA_CYCLES, SIMDS, summary, work          # noqa: E402


def grm_work(n_cols, n_variants, n_cus):
    """bench_ibs.work under hpgv_grm_plan_rows's row ranges: (workgroups, row ranges, k-steps summed over the ranges, blocks)"""
    _, pairs, _, _, blocks = work(n_cols, n_variants, n_cus)
    rows = hpgv.grm_plan_rows(n_variants, n_cols, n_cus)
    splits = -(-n_variants // rows)
    steps = sum(-(-min(rows, n_variants - s * rows) // 64) for s in range(splits))
    return pairs * splits, splits, steps, blocks


def golden(codes, frac_bits, min_maf):
    """{sq, n} int64 [cols, cols, 2] of a code matrix, the table by hpgv_grm_table"""
    hi, lo = codes >> 4, codes & 15
    v = (hi != 15) & (lo != 15)
    g = np.where(v, (hi != 0).astype(np.int64) + (lo != 0), 0)
    c3 = np.stack([(v & (g == c)).sum(axis=1) for c in range(3)], axis=1)
    used, tab = hpgv.grm_table(c3, frac_bits, min_maf)
    q = 256 * tab["hi"].astype(np.int64) + tab["lo"].astype(np.int64)
    V = (v & used[:, None]).astype(np.int64)
    Q = np.take_along_axis(q, g, axis=1) * V
    return np.stack([Q.T @ Q, V.T @ V], axis=-1), int(used.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["10000x100000", "200x1000000"], help="samples x variants")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frac-bits", type=int, default=11)
    ap.add_argument("--min-maf", type=float, default=0.01)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    e = hpgv.Engine(0)
    e.set_option("profile", 1)
    runs = []
    for shape in a.shapes:
        N, V = (int(x) for x in shape.split("x"))
        pitch = -(-N // 16) * 16
        d_gt, d_out = e.alloc(V * pitch), e.alloc(N * N * 16)      # (both tools' records are 16 bytes)
        d_c4, d_skip, d_tab, d_n = e.alloc(V * 16), e.alloc(V + 16), e.alloc(V * 8), e.alloc(16)
        e.synth_raw(0, V, N, pitch, d_gt)
        e.memset_dev(d_skip, 0, V)
        e.ibs_class_counts_dev(d_gt, pitch, V, N, d_c4, d_skip=d_skip)
        e.grm_table_dev(d_c4, V, a.frac_bits, a.min_maf, d_skip, d_tab, d_n)
        e.sync()
        n_used = int(e.d2h(d_n, (1,), np.int32)[0])
        t_grm, t_ibs = [], []
        for r in range(a.warmup + a.iters):
            e.memset_dev(d_out, 0, N * N * 16)
            e.grm_pairs_dev(d_gt, pitch, V, N, d_tab, d_out, d_skip=d_skip)
            e.sync()
            tg = e.last_kernel_ms()[1]
            e.memset_dev(d_out, 0, N * N * 16)
            e.ibs_pairs_dev(d_gt, pitch, V, N, d_out, d_skip=d_skip)
            e.sync()
            ti = e.last_kernel_ms()[1]
            if r >= a.warmup:
                t_grm.append(tg)
                t_ibs.append(ti)
        # a spot check of what was timed: the first 48 columns over the first 3 000 rows, calls of their own, against numpy (the
        # table there is of the 48 columns' own class counts)
        nc, nr = min(N, 48), min(V, 3000)
        d_chk = e.alloc(nc * nc * 16)
        e.memset_dev(d_chk, 0, nc * nc * 16)
        e.memset_dev(d_skip, 0, nr)
        e.ibs_class_counts_dev(d_gt, pitch, nr, nc, d_c4, d_skip=d_skip)
        e.grm_table_dev(d_c4, nr, a.frac_bits, a.min_maf, d_skip, d_tab, d_n)
        e.grm_pairs_dev(d_gt, pitch, nr, nc, d_tab, d_chk, d_skip=d_skip)
        e.sync()
        got = e.d2h(d_chk, (nc, nc, 2), np.int64)
        exp, chk_used = golden(e.d2h(d_gt, (nr, pitch), np.uint8)[:, :nc], a.frac_bits, a.min_maf)
        iu = np.triu_indices(nc)
        ok = bool(np.array_equal(got[iu], exp[iu]) and exp[iu][:, 1].any() and chk_used == int(e.d2h(d_n, (1,), np.int32)[0]))
        for d in (d_gt, d_out, d_c4, d_skip, d_tab, d_n, d_chk):
            e.free(d)
        g, i = summary(t_grm), summary(t_ibs)
        wgs, splits, steps, blocks = grm_work(N, V, a.cus)
        iw = work(N, V, a.cus)
        share = lambda per, st, ms: round(blocks * st * per * MFMA_CYCLES / (SIMDS * ms * 1e-3 * a.clock_ghz * 1e9), 4)
        g.update(workgroups=wgs, row_ranges=splits, rows_per_range=hpgv.grm_plan_rows(V, N, a.cus), mfma=blocks * steps * 5,
                 matrix_pipe_share_at_clock=share(5, steps, g["ms_med"]), pair_variants_per_s=round(N * (N + 1) // 2 * V / (g["ms_med"] * 1e-3), 1))
        i.update(workgroups=iw[0], row_ranges=iw[2], mfma=blocks * iw[3] * 4, matrix_pipe_share_at_clock=share(4, iw[3], i["ms_med"]))
        runs.append(dict(samples=N, variants=V, pitch=pitch, frac_bits=a.frac_bits, min_maf=a.min_maf, rows_used=n_used, k_grm_pairs=g, k_ibs_pairs=i,
                         grm_over_ibs=round(g["ms_med"] / i["ms_med"], 4), sums_equal_numpy_on_first_columns=ok))
    e.close()
    doc = {"bench": "grm_pairs", "iters": a.iters, "warmup": a.warmup, "clock_ghz": a.clock_ghz, "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
