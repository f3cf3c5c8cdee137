#!/usr/bin/env python3
"""Seed items (pcv_searcher_seeds): the device time of one step beside the prep kernel of the same call.

    python tools/bench_seeds.py [--rows 1000000] [--k 64] [--repeats 5] [--warmup 1]

A cosine searcher of --rows x 384 synthetic rows.  For both methods: --warmup calls, then --repeats calls of seeds(k), in one process.
Every call reports prep_ms — selfjoin_prep_kernel, one thread per row reading every f32 row once — and steps_ms, the k picks with
their k - 1 cover steps, each of which reads the same bytes with the same access pattern plus one row (the last pick) in every
thread.  The yardstick is (steps_ms / steps) / prep_ms: about 1 if a cover step costs what the prep kernel costs.  Prints one JSON
line: per method the median and min-max of prep_ms, of the time per step and of their ratio over the repeats, and the bytes per
second of both.  Progress goes to stderr."""
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
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, a.rows, 0x5EED5)
    s.finalize()
    s.wait_background()
    row_bytes = ((a.rows + 31) // 32) * 32 * D * 4
    out = {"metric": "seeds: device ms per step beside prep_ms of the same call", "rows": s.num_rows, "dim": D, "k": a.k, "methods": {}}
    for method in ("kmeans++", "farthest"):
        runs = []
        for i in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            ids, _pos, _totals, _cover = s.seeds(None, a.k, method, seed=i)
            wall = time.perf_counter() - t0
            st = s.last_seed_stats()
            print("%s %s wall %.4f s %s" % (method, "warm-up" if i < a.warmup else "run", wall, st), file=sys.stderr, flush=True)
            if i >= a.warmup:
                runs.append((st["prep_ms"], st["steps_ms"] / max(1, st["steps"]), wall, st["steps"]))
        prep = np.array([r[0] for r in runs])
        step = np.array([r[1] for r in runs])
        out["methods"][method] = {
            "steps": [r[3] for r in runs], "prep_ms": spread(prep), "step_ms": spread(step), "ratio_step_over_prep": spread(step / prep),
            "wall_s": spread([r[2] for r in runs]),
            "prep_bytes_per_s": row_bytes / (float(np.median(prep)) * 1e-3), "step_bytes_per_s": row_bytes / (float(np.median(step)) * 1e-3),
        }
    print(json.dumps(out), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
