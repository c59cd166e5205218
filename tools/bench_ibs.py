#!/usr/bin/env python3
"""The pairwise IBS counts' numbers (DESIGN.md "IBS", k_ibs_pairs): hpgv_ibs_pairs_dev on a resident hpgv_synth_raw_dev matrix at
the shapes samples x variants of --shapes (default 10 000 x 100 000, many tile pairs, and 200 x 1 000 000, ten tile pairs cut into
row ranges).  Kernel times are HIP events around the launch (option "profile"): the median, minimum and maximum of --iters runs
after --warmup, the counts buffer zeroed before each.  Beside the times, computed from the shapes by the kernel's own rules
(work below):
  pair-variants per second  samples (samples - 1) / 2 x variants over the time;
  matrix-pipe share         4 MFMAs per computed 16 x 16 block and k-step x 16 cycles (v_mfma_i32_16x16x64_i8 back to back on one
                            SIMD) over 1 024 SIMDs x time x --clock-ghz, the chip's highest clock: a lower bound of the share at
                            the clock the chip actually held.
For comparison k_ld_window's share from profiles/ld_window.json stands beside it (another contraction, over samples, with six
products).  One JSON document on stdout and in --out."""
import argparse
import json
import os
import sys
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hpgv = import_module("hpg-variant_amd")

SIMDS = 1024
MFMA_CYCLES = 16


def summary(ts):
    med = float(np.median(ts))
    return {"ms_med": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "spread": round((max(ts) - min(ts)) / med, 4)}


def work(n_cols, n_variants, n_cus):
    """what k_ibs_pairs computes by its own rules (ibs_pairs_launch, live[]): (workgroups, row ranges, k-steps summed over the ranges,
    16 x 16 blocks that run MFMAs per k-step)"""
    tiles = -(-n_cols // 64)
    pairs = tiles * (tiles + 1) // 2
    rows = hpgv.ibs_plan_rows(n_variants, n_cols, n_cus)
    splits = -(-n_variants // rows)
    steps = sum(-(-min(rows, n_variants - s * rows) // 64) for s in range(splits))
    blocks = 0
    for tj in range(tiles):
        for ti in range(tj + 1):
            for w in range(4):
                if 64 * ti + 16 * w >= n_cols:
                    continue
                blocks += sum(1 for n in range(4) if 64 * tj + 16 * n < n_cols and (ti != tj or n >= w))
    return pairs * splits, pairs, splits, steps, blocks


def golden(codes):
    hi, lo = codes >> 4, codes & 15
    v = ((hi != 15) & (lo != 15))
    g = np.where(v, (hi != 0).astype(np.int64) + (lo != 0), -1)
    e = [(g == c).astype(np.int64) for c in range(3)]
    vv = v.astype(np.int64)
    n = vv.T @ vv
    ibs0 = e[0].T @ e[2] + e[2].T @ e[0]
    ibs2 = sum(x.T @ x for x in e)
    return np.stack([n, ibs0, n - ibs0 - ibs2, ibs2], axis=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["10000x100000", "200x1000000"], help="samples x variants")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
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
        d_gt, d_counts = e.alloc(V * pitch), e.alloc(N * N * 16)
        e.synth_raw(0, V, N, pitch, d_gt)
        e.sync()
        ts = []
        for r in range(a.warmup + a.iters):
            e.memset_dev(d_counts, 0, N * N * 16)
            e.ibs_pairs_dev(d_gt, pitch, V, N, d_counts)
            e.sync()
            if r >= a.warmup:
                ts.append(e.last_kernel_ms()[1])
        # a spot check of what was timed: the first 48 columns over the first 3 000 rows, a call of its own, against numpy
        nc, nr = min(N, 48), min(V, 3000)
        d_chk = e.alloc(nc * nc * 16)
        e.memset_dev(d_chk, 0, nc * nc * 16)
        e.ibs_pairs_dev(d_gt, pitch, nr, nc, d_chk)
        e.sync()
        got = e.d2h(d_chk, (nc, nc, 4), np.int32)
        exp = golden(e.d2h(d_gt, (nr, pitch), np.uint8)[:, :nc])
        iu = np.triu_indices(nc, 1)
        ok = bool(np.array_equal(got[iu], exp[iu]) and exp[iu][:, 0].any())
        for d in (d_gt, d_counts, d_chk):
            e.free(d)
        s = summary(ts)
        wgs, pairs, splits, steps, blocks = work(N, V, a.cus)
        sec = s["ms_med"] * 1e-3
        pv = N * (N - 1) // 2 * V
        mfma = blocks * steps * 4
        sides = 2 * pairs - -(-N // 64)                              # 64-column blocks the tile pairs load: two each, a diagonal one one
        s.update(samples=N, variants=V, pitch=pitch, workgroups=wgs, tile_pairs=pairs, row_ranges=splits, pair_variants=pv, pair_variants_per_s=round(pv / sec, 1),
                 blocks_per_k_step=blocks, mfma=mfma, matrix_pipe_share_at_clock=round(mfma * MFMA_CYCLES / (SIMDS * sec * a.clock_ghz * 1e9), 4),
                 bytes_requested=int(sides * 64 * V), bytes_requested_over_one_pass=round(sides * 64 / float(pitch), 2),
                 counts_equal_numpy_on_first_columns=ok)
        runs.append(s)
    e.close()
    ld = None
    try:
        with open(os.path.join(ROOT, "profiles", "ld_window.json")) as f:
            ld = {"window_%d" % r["window"]: r["k_ld_window"]["matrix_pipe_share_at_clock"] for r in json.load(f)["runs"]}
    except (OSError, KeyError, ValueError):
        pass
    doc = {"bench": "ibs_pairs", "iters": a.iters, "warmup": a.warmup, "clock_ghz": a.clock_ghz, "runs": runs,
           "k_ld_window_matrix_pipe_share_at_clock": ld}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
