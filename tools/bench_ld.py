#!/usr/bin/env python3
"""The LD band's numbers (DESIGN.md "LD band", k_ld_window): hpgv_ld_window_dev on a resident hpgv_synth_dev matrix of --variants
x --samples in the assoc layout at windows 16, 64 and 256, each beside k_assoc_perm (hpgv_assoc_perm_dev) with n_perms = window
on the same matrix -- the same tile with 2 MFMAs per 16 x 16 block and k-step against 6 -- the two alternating run by run inside
this one process.  Kernel times are HIP events around the launch (option "profile"); per kernel the median, minimum and maximum of
--iters runs after --warmup.  Beside the times, computed from the shapes by the kernel's own rules (blocks_and_bytes below):
  pairs per second          the pairs of the band over the time;
  bytes requested           the genotype bytes the workgroups load (most of them served by L2), against the one-pass minimum
                            variants x pitch;
  matrix-pipe share         6 MFMAs per computed 16 x 16 block and k-step x 16 cycles (v_mfma_i32_16x16x64_i8 back to back on one
                            SIMD) over 1 024 SIMDs x time x --clock-ghz, the chip's highest clock: a lower bound of the share at
                            the clock the chip actually held.
One JSON document on stdout and in --out."""
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


def blocks_and_bytes(V, window, pitch):
    """what k_ld_window computes and loads for b_begin = 0, by its own rules: (16 x 16 blocks that run MFMAs, bytes loaded)"""
    tiles, passes = -(-V // 64), (63 + window) // 64 + 1
    blocks = rows = 0
    for t in range(tiles):
        for p in range(passes):
            a0, b0 = 64 * t, 64 * t + 64 * p
            if b0 >= V:
                continue
            for w in range(4):
                aw = a0 + 16 * w
                live = sum(1 for n in range(4) if b0 + 16 * n + 15 > aw and b0 + 16 * n <= aw + 15 + window and b0 + 16 * n < V and aw < V)
                blocks += live
                rows += min(16, max(0, V - aw)) if live else 0
            rows += min(64, V - b0)
    return blocks, rows * pitch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--windows", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    V, N = a.variants, a.samples
    e = hpgv.Engine(0)
    cond = (np.arange(N) % 2).astype(np.uint8)
    _, _, pitch = e.set_cohort(cond)
    d_gt, d_c4, d_nge = e.alloc(V * pitch), e.alloc(V * 16), e.alloc(V * 4)
    e.synth(hpgv.LAYOUT_ASSOC, 0, V, d_gt)
    e.assoc_scan(d_gt, V, d_c4)
    e.sync()
    e.set_option("profile", 1)
    steps = -(-(pitch // 16) // 4)
    runs = []
    for W in a.windows:
        e.set_perm_labels(hpgv.perm_labels_shuffle(cond, W, a.seed))
        d_r2, d_max = e.alloc(V * W * 8), e.alloc(W * 8)

        def ld():
            e.ld_window_dev(d_gt, pitch, V, W, d_r2); e.sync()
            return e.last_kernel_ms()[1]

        def perm():
            e.assoc_perm_dev(d_gt, V, d_c4, d_nge, d_max); e.sync()
            return e.last_kernel_ms()[1]

        tl, tp = [], []
        for r in range(a.warmup + a.iters):
            x, y = ld(), perm()
            if r >= a.warmup:
                tl.append(x); tp.append(y)
        # a spot check of what was timed: the first rows' band against the host function on counts of a second, small call
        n_chk = min(V, 200)
        d_c6 = e.alloc(n_chk * W * 48)
        e.ld_window_dev(d_gt, pitch, n_chk, W, d_r2, d_c6); e.sync()
        r2, c6 = e.d2h(d_r2, (n_chk, W), np.float64), e.d2h(d_c6, (n_chk, W, 6), np.int32)
        ref = hpgv.ld_r2(c6)
        ok = bool(np.array_equal(np.isnan(r2), np.isnan(ref)) and np.array_equal(r2[~np.isnan(ref)], ref[~np.isnan(ref)]) and np.isfinite(r2).any())
        for d in (d_r2, d_max, d_c6):
            e.free(d)
        sl, sp = summary(tl), summary(tp)
        pairs = sum(min(W, b) for b in range(min(V, W))) + max(0, V - W) * W
        blocks, loaded = blocks_and_bytes(V, W, pitch)
        sec = sl["ms_med"] * 1e-3
        sl.update(pairs=pairs, pairs_per_s=round(pairs / sec, 1), blocks_computed=blocks,
                  share_of_blocks_inside_the_band=round(pairs / (blocks * 256.0), 4),
                  bytes_requested=loaded, bytes_requested_over_one_pass=round(loaded / float(V * pitch), 3),
                  mfma=blocks * steps * 6, matrix_pipe_share_at_clock=round(blocks * steps * 6 * MFMA_CYCLES / (SIMDS * sec * a.clock_ghz * 1e9), 4),
                  r2_is_ld_r2_of_counts6_on_first_rows=ok)
        pblocks = -(-V // 64) * 4 * (-(-W // 128) * 8)            # a wave runs all 8 blocks of a pass, whatever n_perms is
        psec = sp["ms_med"] * 1e-3
        sp.update(n_perms=W, blocks_computed=pblocks, mfma=pblocks * steps * 2,
                  matrix_pipe_share_at_clock=round(pblocks * steps * 2 * MFMA_CYCLES / (SIMDS * psec * a.clock_ghz * 1e9), 4))
        runs.append({"window": W, "k_ld_window": sl, "k_assoc_perm": sp, "ld_over_perm_time": round(sl["ms_med"] / sp["ms_med"], 4),
                     "ld_over_perm_mfma": round(sl["mfma"] / float(sp["mfma"]), 4)})
    e.close()
    doc = {"bench": "ld_window", "variants": V, "samples": N, "pitch": pitch, "k_steps": steps, "iters": a.iters, "warmup": a.warmup,
           "clock_ghz": a.clock_ghz, "one_pass_bytes": V * pitch, "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
