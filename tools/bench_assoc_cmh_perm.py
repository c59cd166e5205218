#!/usr/bin/env python3
"""The numbers of the permutation within strata (DESIGN.md "Stratified association", k_assoc_cmh_perm): on a resident matrix of
--shapes (samples x rows), --perms label rows and --strata strata,
  (1) hpgv_assoc_cmh_perm_dev with stratum-contiguous columns (every stratum a block of each class, so a block of the assoc layout)
      and with interleaved columns (a random stratum per column), the label rows shuffled within the strata;
  (2) hpgv_assoc_perm_dev at the same number of permutations, from the same build: the floor, the same product without strata;
  (3) route (b), the way to within-stratum counts before this call: perms x K label rows, each a label row masked to one stratum,
      through hpgv_set_perm_labels, and hpgv_assoc_perm_dev with d_perm_counts -- V x perms x K x 2 integers and no statistic.
      It uses nothing this call added, so it runs from a build of the commit before it: --parent-root names such a checkout
      (built); this file is run there as a child process with --root.  Without --parent-root it is measured on this tree.  Where
      its label image or its counts do not fit the device the record says so instead of a time.
Kernel times are HIP events around the launch (option "profile"); per figure the median, minimum and maximum of --iters runs
after --warmup.  The matrix is a block of random rows laid out on the device and repeated.  A line of progress per figure on
stderr; one JSON document on stdout and in --out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
from importlib import import_module

import numpy as np

BLOCK_ROWS = 4096


def summary(ts):
    med = float(np.median(ts))
    return {"ms_med": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "spread": round((max(ts) - min(ts)) / med, 4)}


def timed(a, run, what):
    ts = [run() for _ in range(a.warmup + a.iters)][a.warmup:]
    s = summary(ts)
    print("%s: %s" % (what, s), file=sys.stderr, flush=True)
    return s


def resident_matrix(hpgv, e, N, V, missing, seed):
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


def strata_of(N, K, order, seed):
    """the stratum of every column: `contiguous` = blocks of each class (cond alternates, so column j is number j // 2 of its class)"""
    if order == "contiguous":
        return ((np.arange(N) // 2) * K // ((N + 1) // 2)).astype(np.int32)
    return np.random.default_rng(seed + K).integers(0, K, N).astype(np.int32)


def plain_rows(N, P, seed):
    """P label rows, fair coins: what they hold does not change the work of (2) and (3)"""
    return (np.random.default_rng(seed + 7).random((P, N)) < 0.5).astype(np.uint8)


def one_shape(hpgv, a, N, V, route):
    out = []
    cond = (np.arange(N) % 2).astype(np.uint8)
    e = hpgv.Engine(0)
    e.set_cohort(cond)
    d_gt, pitch = resident_matrix(hpgv, e, N, V, a.missing, a.seed)
    e.set_option("profile", 1)
    base = {"samples": N, "rows": V, "pitch": pitch, "missing": a.missing, "perms": a.perms}
    d_nge = e.alloc(V * 4)
    if route == "new":
        # (2) the floor
        e.set_perm_labels(plain_rows(N, a.perms, a.seed))
        d_c4, d_max = e.alloc(V * 16), e.alloc(a.perms * 8)
        e.assoc_scan(d_gt, V, d_c4)
        e.sync()

        def floor():
            e.assoc_perm_dev(d_gt, V, d_c4, d_nge, d_max); e.sync()
            return e.last_kernel_ms()[1]

        fl = timed(a, floor, "%dx%d floor" % (N, V))
        for K in a.strata:
            rec = dict(base, strata=K, floor_hpgv_assoc_perm_dev=fl)
            d_out, d_tab = e.alloc(V * 72), e.alloc(V * K * 16)
            for order in ("contiguous", "interleaved"):
                stratum = strata_of(N, K, order, a.seed)
                e.set_strata(stratum, K)
                e.set_perm_labels(hpgv.perm_labels_shuffle_within(cond, stratum, a.perms, a.seed))
                e.assoc_cmh_dev(d_gt, V, d_out, d_tab)
                e.sync()

                def run():
                    e.assoc_cmh_perm_dev(d_gt, V, d_tab, d_nge, d_max); e.sync()
                    return e.last_kernel_ms()[1]

                rec[order] = timed(a, run, "%dx%d K=%d %s" % (N, V, K, order))
                rec[order + "_over_floor"] = round(rec[order]["ms_med"] / fl["ms_med"], 3)
            e.free(d_out); e.free(d_tab)
            out.append(rec)
    else:
        rows = plain_rows(N, a.perms, a.seed)
        for K in a.strata:
            rec = dict(base, strata=K)
            stratum = strata_of(N, K, "interleaved", a.seed)
            label_bytes, count_bytes = a.perms * K * pitch, V * a.perms * K * 8
            rec["route_b_label_bytes"], rec["route_b_count_bytes"] = label_bytes, count_bytes
            try:
                masked = np.concatenate([rows & (stratum == k) for k in range(K)])      # [K x perms, N]
                e.set_perm_labels(masked)
                del masked
                d_c4, d_max, d_pc = e.alloc(V * 16), e.alloc(a.perms * K * 8), e.alloc(count_bytes)
            except (hpgv.HpgvError, MemoryError) as err:
                rec["route_b"] = "does not fit: %s" % str(err)[:120]
                out.append(rec)
                continue
            e.assoc_scan(d_gt, V, d_c4)
            e.sync()

            def run():
                e.assoc_perm_dev(d_gt, V, d_c4, d_nge, d_max, d_pc); e.sync()
                return e.last_kernel_ms()[1]

            rec["route_b"] = timed(a, run, "%dx%d K=%d route (b)" % (N, V, K))
            for b in (d_c4, d_max, d_pc):
                e.free(b)
            out.append(rec)
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000x4096,200x65536", help="samples x rows, comma-separated")
    ap.add_argument("--strata", default="2,8,64")
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--route", choices=["new", "b"], default="new")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose package and build are measured")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit before the call: (3) is measured there")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    hpgv = import_module("hpg-variant_amd")
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    a.strata = [int(x) for x in a.strata.split(",")]
    runs = [r for N, V in shapes for r in one_shape(hpgv, a, N, V, a.route)]
    doc = {"bench": "assoc_cmh_perm", "route": a.route, "iters": a.iters, "warmup": a.warmup, "runs": runs}
    if a.route == "new":
        if a.parent_root:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", "b", "--root", a.parent_root, "--shapes", a.shapes,
                                    "--strata", ",".join(map(str, a.strata)), "--perms", str(a.perms), "--missing", str(a.missing),
                                    "--iters", str(a.iters), "--warmup", str(a.warmup), "--seed", str(a.seed)], stdout=subprocess.PIPE, text=True, check=True)
            other, where = json.loads(child.stdout)["runs"], "parent checkout"
        else:
            other, where = [r for N, V in shapes for r in one_shape(hpgv, a, N, V, "b")], "this tree"
        doc["route_b_measured_on"] = where
        for r, o in zip(runs, other):
            assert (r["samples"], r["rows"], r["strata"]) == (o["samples"], o["rows"], o["strata"])
            r.update({k: o[k] for k in ("route_b", "route_b_label_bytes", "route_b_count_bytes")})
            if isinstance(o["route_b"], dict):
                for order in ("contiguous", "interleaved"):
                    r["route_b_over_" + order] = round(o["route_b"]["ms_med"] / r[order]["ms_med"], 3)
                    # the expectation: faster by more than the run-to-run spread of both
                    r[order + "_beats_route_b"] = bool(r[order]["ms_max"] < o["route_b"]["ms_min"])
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
