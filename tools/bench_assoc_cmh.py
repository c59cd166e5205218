#!/usr/bin/env python3
"""The stratified association's numbers (DESIGN.md "Kernels", k_assoc_cmh_tables and k_assoc_cmh_stats): hpgv_assoc_cmh_dev on a
resident matrix of --shapes (samples x rows) for --strata strata with --missing fractions of missing calls, each beside
  (a) hpgv_read_probe of the same matrix: the time of a plain read, and
  (b) the route to the same integers without the tool: hpgv_set_perm_labels with the 2K stratum indicator rows as "labels", then
      hpgv_assoc_perm_dev with d_perm_counts.  --route perm measures (b) alone and uses nothing this tool added, so the same file
      runs in a checkout of the commit before it: --parent-root names such a checkout (built), whose own copy of this file is run
      as a child process and whose figures land beside the new call's.  Without it (b) is measured on this tree.
Kernel times are HIP events around the launches (option "profile": tables + records for the new call, the permutation kernel
for (b)); per figure the median, minimum and maximum of --iters runs after --warmup.  The matrix is a block of random rows laid
out on the device and repeated.  One JSON document on stdout and in --out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hpgv = import_module("hpg-variant_amd")

BLOCK_ROWS = 4096


def summary(ts):
    med = float(np.median(ts))
    return {"ms_med": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "spread": round((max(ts) - min(ts)) / med, 4)}


def timed(a, run):
    ts = []
    for r in range(a.warmup + a.iters):
        t = run()
        if r >= a.warmup:
            ts.append(t)
    return summary(ts)


def resident_matrix(e, N, V, missing, seed):
    """V rows of N random calls in the assoc layout on the device: (d_gt, pitch)"""
    rng = np.random.default_rng(seed)
    rows = min(V, BLOCK_ROWS)
    p = np.array([0.45, 0.35, 0.2])
    block = np.array([0x00, 0x01, 0x11, 0xFF], np.uint8)[rng.choice(4, size=(rows, N), p=np.append(p * (1.0 - missing), missing))]
    pitch = e.assoc_layout()[2]
    d_raw, d_gt = e.alloc(V * N), e.alloc(V * pitch)
    for v0 in range(0, V, rows):
        n = min(rows, V - v0)
        e.h2d(C.c_void_p(d_raw.value + v0 * N), block[:n])
    e.layout(hpgv.LAYOUT_ASSOC, d_raw, N, V, d_gt)
    e.sync()
    e.free(d_raw)
    return d_gt, pitch


def one_shape(a, N, V, route):
    out = []
    cond = (np.arange(N) % 2).astype(np.uint8)
    for missing in a.missing:
        e = hpgv.Engine(0)
        e.set_cohort(cond)
        d_gt, pitch = resident_matrix(e, N, V, missing, a.seed)
        e.set_option("profile", 1)
        probe = e.read_probe(d_gt, V * pitch, a.iters)
        for K in a.strata:
            stratum = (np.random.default_rng(a.seed + K).integers(0, K, N)).astype(np.int32)
            rec = {"samples": N, "rows": V, "pitch": pitch, "bytes": V * pitch, "missing": missing, "strata": K, "read_probe_ms": round(probe, 4)}
            if route == "cmh":
                e.set_strata(stratum, K)
                d_out, d_tab = e.alloc(V * 72), e.alloc(V * K * 16)

                def run():
                    e.assoc_cmh_dev(d_gt, V, d_out, d_tab); e.sync()
                    return e.last_kernel_ms()

                both = [run() for _ in range(a.warmup + a.iters)][a.warmup:]
                rec["tables"] = summary([t[0] for t in both])
                rec["records"] = summary([t[1] for t in both])
                rec["hpgv_assoc_cmh_dev"] = summary([t[0] + t[1] for t in both])
                rec["over_read_probe"] = round(rec["hpgv_assoc_cmh_dev"]["ms_med"] / probe, 3)
                rec["tables_gb_per_s"] = round(V * pitch / (rec["tables"]["ms_med"] * 1e-3) / 1e9, 1)
                e.free(d_out); e.free(d_tab)
                e.set_strata(None)
            else:
                labels = np.zeros((2 * K, N), np.uint8)
                for k in range(K):
                    labels[2 * k] = (stratum == k) & (cond == 1)
                    labels[2 * k + 1] = (stratum == k) & (cond == 0)
                e.set_perm_labels(labels)
                d_c4, d_nge, d_max, d_pc = e.alloc(V * 16), e.alloc(V * 4), e.alloc(2 * K * 8), e.alloc(V * 2 * K * 8)
                e.assoc_scan(d_gt, V, d_c4)
                e.sync()

                def run():
                    e.assoc_perm_dev(d_gt, V, d_c4, d_nge, d_max, d_pc); e.sync()
                    return e.last_kernel_ms()[1]

                rec["hpgv_assoc_perm_dev"] = timed(a, run)
                for b in (d_c4, d_nge, d_max, d_pc):
                    e.free(b)
                e.set_perm_labels(None)
            out.append(rec)
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000x65536,200x4000000", help="samples x rows, comma-separated")
    ap.add_argument("--strata", default="2,8,32,64,200")
    ap.add_argument("--missing", default="0,0.02")
    ap.add_argument("--route", choices=["cmh", "perm"], default="cmh")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit before the tool, holding a copy of this file: (b) is measured there")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    a.strata = [int(x) for x in a.strata.split(",")]
    a.missing = [float(x) for x in a.missing.split(",")]
    runs = [r for N, V in shapes for r in one_shape(a, N, V, a.route)]
    doc = {"bench": "assoc_cmh", "route": a.route, "iters": a.iters, "warmup": a.warmup, "runs": runs}
    if a.route == "cmh":
        if a.parent_root:
            child = subprocess.run([sys.executable, os.path.join(a.parent_root, "tools", "bench_assoc_cmh.py"), "--route", "perm", "--shapes", a.shapes,
                                    "--strata", ",".join(map(str, a.strata)), "--missing", ",".join(map(str, a.missing)), "--iters", str(a.iters),
                                    "--warmup", str(a.warmup), "--seed", str(a.seed)], capture_output=True, text=True, check=True)
            other, where = json.loads(child.stdout)["runs"], "parent checkout"
        else:
            other, where = [r for N, V in shapes for r in one_shape(a, N, V, "perm")], "this tree"
        doc["route_b_measured_on"] = where
        for r, o in zip(runs, other):
            assert (r["samples"], r["rows"], r["missing"], r["strata"]) == (o["samples"], o["rows"], o["missing"], o["strata"])
            r["route_b_hpgv_assoc_perm_dev"] = o["hpgv_assoc_perm_dev"]
            r["route_b_over_cmh"] = round(o["hpgv_assoc_perm_dev"]["ms_med"] / r["hpgv_assoc_cmh_dev"]["ms_med"], 3)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
