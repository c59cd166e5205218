#!/usr/bin/env python3
"""The label permutation kernel's numbers (DESIGN.md "Kernels", k_assoc_perm) on a synthetic cohort (hpgv_synth_dev, assoc
layout): hpgv_assoc_perm_dev on --variants x --samples rows (half affected, half unaffected) with 64 and with 1 024 label
rows of hpgv_perm_labels_shuffle.  Per run: the kernel time (HIP events around the launch, median of --iters after --warmup
launches of the same shape), the rate in multiply-accumulates (variants x row bytes x permutations x 2 planes) per second,
and that rate as a share of the i8 dense peak (twice the BF16 rate: 5e15 operations = 2.5e15 MAC per second).
From the two runs, the epilogue's share: a launch costs passes x variants x row bytes x m (the k-loop; passes = ceil(P / 128)
tiles of permutations) + variants x P x e (the f64 epilogue, per valid permutation); 64 permutations are one pass, 1 024 are
eight, which gives m and e.  Results as one JSON document on stdout and in --out."""
import argparse
import json
import os
import sys
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hpgv = import_module("hpg-variant_amd")
I8_PEAK_MACS = 2.5e15
TILE = 128


def run(e, cond, d_gt, d_counts, V, pitch, P, a):
    e.set_perm_labels(hpgv.perm_labels_shuffle(cond, P, a.seed))
    d_nge, d_max = e.alloc(V * 4), e.alloc(P * 8)
    ts = []
    for r in range(a.warmup + a.iters):
        e.assoc_perm_dev(d_gt, V, d_counts, d_nge, d_max)
        e.sync()
        if r >= a.warmup:
            ts.append(e.last_kernel_ms()[1])
    bmax = e.d2h(d_max, (P,), np.float64)
    e.free(d_nge); e.free(d_max)
    med = float(np.median(ts))
    macs = V * pitch * P * 2
    return {"permutations": P, "passes_over_genotypes": -(-P // TILE), "ms_med": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
            "macs": macs, "macs_per_s": macs / (med * 1e-3), "frac_i8_dense_peak": round(macs / (med * 1e-3) / I8_PEAK_MACS, 5),
            "batch_max_mean": float(bmax.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=32768)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    V, N = a.variants, a.samples
    e = hpgv.Engine(0)
    cond = (np.arange(N) % 2).astype(np.uint8)
    _, _, pitch = e.set_cohort(cond)
    d_gt, d_counts = e.alloc(V * pitch), e.alloc(V * 16)
    e.synth(hpgv.LAYOUT_ASSOC, 0, V, d_gt)
    e.assoc_scan(d_gt, V, d_counts)
    e.sync()
    e.set_option("profile", 1)
    small, large = run(e, cond, d_gt, d_counts, V, pitch, 64, a), run(e, cond, d_gt, d_counts, V, pitch, 1024, a)
    e.close()
    # t(P) = passes(P) * loop + V * P * e_per_pair:  t64 = loop + 64 V e,  t1024 = 8 loop + 1024 V e
    t64, t1024 = small["ms_med"], large["ms_med"]
    epi_pair_ms = (t1024 - 8 * t64) / (V * (1024 - 8 * 64))
    loop_pass_ms = t64 - V * 64 * epi_pair_ms
    doc = {"bench": "assoc_perm", "variants": V, "samples": N, "pitch": pitch, "iters": a.iters, "warmup": a.warmup,
           "i8_dense_peak_macs_per_s": I8_PEAK_MACS, "runs": [small, large],
           "model": {"loop_ms_per_pass": round(loop_pass_ms, 4), "epilogue_ns_per_variant_permutation": round(epi_pair_ms * 1e6, 5),
                     "epilogue_share_at_64": round(V * 64 * epi_pair_ms / t64, 4), "epilogue_share_at_1024": round(V * 1024 * epi_pair_ms / t1024, 4)}}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
