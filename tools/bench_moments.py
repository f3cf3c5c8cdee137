#!/usr/bin/env python3
"""Corpus moments and projection (pcv_searcher_moments, _project): device times beside the prep kernel of the same call.

    python tools/bench_moments.py [--rows 1000000] [--repeats 5] [--warmup 1]

A cosine searcher of --rows x 384 synthetic rows.  --warmup calls, then --repeats calls, in one process, of moments(centered) and of
project with m = 2 and m = 64 random axes.  moments reports prep_ms (selfjoin_prep_kernel, one thread per row reading every f32 row
once), sums_ms and syrk_ms, the three limb matrices on the f64 MFMA: 3 * 2 * n * Dp^2 FLOP, each symmetric matrix counted as half.
project reports prep_ms and project_ms, which reads the same bytes once per group of 8 axes (2 for m <= 2).  Prints one JSON line:
the median and min-max of every time over the repeats, the f64 FLOP/s syrk_ms implies and project_ms / prep_ms.  Progress goes to
stderr."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import perceive_amd as pa  # noqa: E402

D = 384


def spread(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, a.rows, 0x5EED5)
    s.finalize()
    s.wait_background()
    Dp = (D + 63) // 64 * 64
    out = {"metric": "moments and project: device ms beside prep_ms of the same call", "rows": s.num_rows, "dim": D}
    runs = []
    for i in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        _sums, _mat, n = s.moments(None, centered=True)
        wall = time.perf_counter() - t0
        st = s.last_moment_stats()
        print("moments %s wall %.4f s %s" % ("warm-up" if i < a.warmup else "run", wall, st), file=sys.stderr, flush=True)
        if i >= a.warmup:
            runs.append((st["prep_ms"], st["sums_ms"], st["syrk_ms"], wall))
    syrk = np.array([r[2] for r in runs])
    flop = 3.0 * 2.0 * n * Dp * Dp
    out["moments"] = {
        "participating": n, "tile_features": st["tile_features"], "row_ranges": st["row_ranges"],
        "prep_ms": spread([r[0] for r in runs]), "sums_ms": spread([r[1] for r in runs]), "syrk_ms": spread(syrk),
        "syrk_f64_flop_per_s": spread(flop / (syrk * 1e-3)), "wall_s": spread([r[3] for r in runs]),
    }
    rng = np.random.default_rng(1)
    out["project"] = {}
    for m in (2, 64):
        axes = rng.standard_normal((m, D)).astype(np.float32)
        runs = []
        for i in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            s.project(None, axes)
            wall = time.perf_counter() - t0
            st = s.last_project_stats()
            print("project m=%d %s wall %.4f s %s" % (m, "warm-up" if i < a.warmup else "run", wall, st), file=sys.stderr, flush=True)
            if i >= a.warmup:
                runs.append((st["prep_ms"], st["project_ms"], wall))
        prep, proj = np.array([r[0] for r in runs]), np.array([r[1] for r in runs])
        out["project"]["m%d" % m] = {"prep_ms": spread(prep), "project_ms": spread(proj), "ratio_project_over_prep": spread(proj / prep),
                                     "wall_s": spread([r[2] for r in runs])}
    print(json.dumps(out), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
