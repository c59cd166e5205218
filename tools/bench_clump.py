#!/usr/bin/env python3
"""The edge form of the LD band beside the band form (DESIGN.md "LD band", k_ld_edges / k_ld_window): hpgv_ld_edges_dev and
hpgv_ld_window_dev (without counts6) on the same resident hpgv_synth_dev matrix of --variants x --samples in the assoc layout, at
windows 16, 64 and 256, the two alternating run by run inside this one process.  The edge form runs at min_r2 = 0.5 (a clumping
threshold: next to no pair of the synthetic matrix qualifies, so the epilogue is ballots alone) and at min_r2 = 0 (every pair with a
finite r2 is emitted: the worst case for the append).  Kernel times are HIP events around the launch (option "profile"; the edge
form's include the 8-byte memset of its counter); per kernel the median, minimum and maximum of --iters runs after --warmup.  Beside
the times, from the shapes: the bytes each form writes (band: 8 per pair of the band, written or NaN; edges: 16 per emitted pair)
and the edge form's adds (at most one per wave, 16 x 16 block and accumulator register that holds a qualifying pair; the count
given is the upper bound blocks x 4).  One JSON document on stdout and in --out."""
import argparse
import json
import os
import sys
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
hpgv = import_module("hpg-variant_amd")
from bench_ld import blocks_and_bytes, summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--windows", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--min-r2", type=float, nargs="+", default=[0.5, 0.0])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    V, N = a.variants, a.samples
    e = hpgv.Engine(0)
    cond = (np.arange(N) % 2).astype(np.uint8)
    _, _, pitch = e.set_cohort(cond)
    d_gt = e.alloc(V * pitch)
    e.synth(hpgv.LAYOUT_ASSOC, 0, V, d_gt)
    e.sync()
    e.set_option("profile", 1)
    runs = []
    for W in a.windows:
        pairs = sum(min(W, b) for b in range(min(V, W))) + max(0, V - W) * W
        blocks, _ = blocks_and_bytes(V, W, pitch)
        d_r2, d_edges, d_n = e.alloc(V * W * 8), e.alloc(pairs * 16 + 16), e.alloc(16)

        def band():
            e.ld_window_dev(d_gt, pitch, V, W, d_r2); e.sync()
            return e.last_kernel_ms()[1]

        def edges(m):
            e.ld_edges_dev(d_gt, pitch, V, W, m, d_edges, pairs, d_n); e.sync()
            return e.last_kernel_ms()[1]

        tb, te = [], {m: [] for m in a.min_r2}
        for r in range(a.warmup + a.iters):
            x = band()
            ys = {m: edges(m) for m in a.min_r2}
            if r >= a.warmup:
                tb.append(x)
                for m in a.min_r2:
                    te[m].append(ys[m])
        r2 = e.d2h(d_r2, (V, W), np.float64)
        sb = summary(tb)
        sb.update(pairs=pairs, bytes_written=V * W * 8)
        run = {"window": W, "blocks_computed": blocks, "k_ld_window": sb, "k_ld_edges": []}
        for m in a.min_r2:
            edges(m)
            count = int(e.d2h(d_n, (1,), np.uint64)[0])
            with np.errstate(invalid="ignore"):
                expect = int((r2 >= m).sum())
            s = summary(te[m])
            s.update(min_r2=m, edges=count, count_is_the_bands=bool(count == expect), bytes_written=count * 16, adds_at_most=min(blocks * 4, count),
                     edges_over_band_time=round(s["ms_med"] / sb["ms_med"], 4), faster="edges" if s["ms_med"] < sb["ms_med"] else "band")
            run["k_ld_edges"].append(s)
        runs.append(run)
        for d in (d_r2, d_edges, d_n):
            e.free(d)
    e.close()
    doc = {"bench": "ld_edges", "variants": V, "samples": N, "pitch": pitch, "iters": a.iters, "warmup": a.warmup, "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
