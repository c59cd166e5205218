#!/usr/bin/env python3
"""The model tests' numbers (DESIGN.md "Kernels", k_assoc_model_scan and the trend form of k_assoc_perm), each beside the
existing kernel it is measured against, the two alternating run by run inside this one process:
  1. the resident class scan (hpgv_assoc_model_scan_dev) against the allelic scan (hpgv_assoc_scan_dev, k_assoc_scan_pipe) on
     the same hpgv_synth_dev matrix of --variants x --samples;
  2. the trend form of the permutation kernel (hpgv_assoc_trend_perm_dev) against the allelic form (hpgv_assoc_perm_dev) on
     --perm-variants x --perm-samples with 64 and with 1 024 label rows, the shape of tools/bench_assoc_perm.py;
  3. one hpgv_assoc_model_text call against one hpgv_assoc_text call (task CHISQ) on the same text of --text-lines x
     --text-samples (host wall time of the synchronous call: copy, tokenizer, layout, kernels, copies back).
Kernel times are HIP events around the launch (option "profile"); per pair the median, minimum and maximum of --iters runs after
--warmup, and the spread (max - min) / median of each.  One JSON document on stdout and in --out."""
import argparse
import json
import os
import sys
import time
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hpgv = import_module("hpg-variant_amd")


def summary(ts, extra=None):
    med = float(np.median(ts))
    d = {"ms_med": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "spread": round((max(ts) - min(ts)) / med, 4)}
    d.update(extra(med) if extra else {})
    return d


def alternate(a, first, second):
    """first and second are callables returning one time in ms; they run in turn, first, second, first, ..."""
    t1, t2 = [], []
    for r in range(a.warmup + a.iters):
        x, y = first(), second()
        if r >= a.warmup:
            t1.append(x); t2.append(y)
    return t1, t2


def scans(a):
    V, N = a.variants, a.samples
    e = hpgv.Engine(0)
    cond = (np.arange(N) % 2).astype(np.uint8)
    _, _, pitch = e.set_cohort(cond)
    d_gt, d_c4, d_c8 = e.alloc(V * pitch), e.alloc(V * 16), e.alloc(V * 32)
    e.synth(hpgv.LAYOUT_ASSOC, 0, V, d_gt)
    e.sync()
    e.set_option("profile", 1)

    def allelic():
        e.assoc_scan(d_gt, V, d_c4); e.sync()
        return e.last_kernel_ms()[0]

    def model():
        e.assoc_model_scan(d_gt, V, d_c8); e.sync()
        return e.last_kernel_ms()[0]

    ta, tm = alternate(a, allelic, model)
    c4, c8 = e.d2h(d_c4, (V, 4), np.int32), e.d2h(d_c8, (V, 8), np.int32)
    same = bool(np.array_equal(2 * c8[:, 0] + c8[:, 1], c4[:, 0]) and np.array_equal(c8[:, 1] + 2 * c8[:, 2], c4[:, 1]) and
                np.array_equal(2 * c8[:, 3] + c8[:, 4], c4[:, 2]) and np.array_equal(c8[:, 4] + 2 * c8[:, 5], c4[:, 3]))
    e.close()
    rate = lambda med: {"gb_per_s": round(V * pitch / (med * 1e-3) / 1e9, 1)}
    sa, sm = summary(ta, rate), summary(tm, rate)
    return {"variants": V, "samples": N, "pitch": pitch, "bytes": V * pitch, "k_assoc_scan_pipe": sa, "k_assoc_model_scan": sm,
            "model_over_allelic_rate": round(sm["gb_per_s"] / sa["gb_per_s"], 4), "allele_count_identity_holds": same}


def perms(a):
    V, N = a.perm_variants, a.perm_samples
    e = hpgv.Engine(0)
    cond = (np.arange(N) % 2).astype(np.uint8)
    _, _, pitch = e.set_cohort(cond)
    d_gt, d_c4, d_c8, d_nge = e.alloc(V * pitch), e.alloc(V * 16), e.alloc(V * 32), e.alloc(V * 4)
    e.synth(hpgv.LAYOUT_ASSOC, 0, V, d_gt)
    e.assoc_scan(d_gt, V, d_c4)
    e.assoc_model_scan(d_gt, V, d_c8)
    e.sync()
    e.set_option("profile", 1)
    runs = []
    for P in (64, 1024):
        e.set_perm_labels(hpgv.perm_labels_shuffle(cond, P, a.seed))
        d_max = e.alloc(P * 8)

        def allelic():
            e.assoc_perm_dev(d_gt, V, d_c4, d_nge, d_max); e.sync()
            return e.last_kernel_ms()[1]

        def trend():
            e.assoc_trend_perm_dev(d_gt, V, d_c8, d_nge, d_max); e.sync()
            return e.last_kernel_ms()[1]

        ta, tt = alternate(a, allelic, trend)
        e.free(d_max)
        sa, st = summary(ta), summary(tt)
        runs.append({"permutations": P, "allelic": sa, "trend": st, "trend_over_allelic_time": round(st["ms_med"] / sa["ms_med"], 4)})
    e.close()
    return {"variants": V, "samples": N, "pitch": pitch, "runs": runs}


def texts(a):
    L, N = a.text_lines, a.text_samples
    rng = np.random.default_rng(a.seed)
    cells = np.array([b"0/0\t", b"0/1\t", b"1/1\t", b"./.\t"], dtype="S4")[rng.choice(4, size=(L, N), p=[0.45, 0.35, 0.17, 0.03])]
    text = b"".join(b"7\t%d\trs%d\tA\tC\t.\tPASS\t.\tGT\t" % (100 + v, v) + cells[v].tobytes()[:-1] + b"\n" for v in range(L))
    e = hpgv.Engine(0)
    e.set_cohort((np.arange(N) % 2).astype(np.uint8))

    def timed(f):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3

    ta, tm = alternate(a, lambda: timed(lambda: e.assoc_text(hpgv.TASK_CHISQ, text, L)), lambda: timed(lambda: e.assoc_model_text(text, L)))
    e.close()
    sa, sm = summary(ta), summary(tm)
    return {"lines": L, "samples": N, "text_bytes": len(text), "hpgv_assoc_text": sa, "hpgv_assoc_model_text": sm,
            "model_over_assoc_time": round(sm["ms_med"] / sa["ms_med"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=1000000)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--perm-variants", type=int, default=32768)
    ap.add_argument("--perm-samples", type=int, default=4096)
    ap.add_argument("--text-lines", type=int, default=4096)
    ap.add_argument("--text-samples", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = {"bench": "assoc_model", "iters": a.iters, "warmup": a.warmup, "scan": scans(a), "perm": perms(a), "text": texts(a)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
