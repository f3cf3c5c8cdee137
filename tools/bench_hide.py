#!/usr/bin/env python3
"""Hidden items (pcv_searcher_hide_ids): what hiding and unhiding cost, and what hidden rows do to a search step.

    python tools/bench_hide.py [--explicit-rows 10000000] [--synthetic-rows 100000000] [--steps 20]

Prints one JSON object:
  explicit   hide / unhide latency (ms, median of 3) for 1 / 1 000 / 100 000 ids on a corpus with an id column (add_rows; the
             rows are copies of one 1M-row chunk under distinct ids: content does not matter to the id match)
  synthetic  the same on synthetic rows (implicit ids: found by arithmetic on the host)
  step       the 64-query top-10 step on the synthetic corpus before and after hiding 1 % of its rows: wall ms (median of
             --steps), device total_ms, coarse_survivors of last_stats()
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import perceive_amd as pa  # noqa: E402

D = 384


def latency(s, pick, n, rng, reps=3):
    hide, unhide = [], []
    for _ in range(reps):
        ids = pick(n, rng)
        t0 = time.perf_counter()
        s.hide_items(ids)
        t1 = time.perf_counter()
        s.unhide_items(ids)
        t2 = time.perf_counter()
        hide.append((t1 - t0) * 1e3)
        unhide.append((t2 - t1) * 1e3)
    return {"ids": n, "hide_ms": float(np.median(hide)), "unhide_ms": float(np.median(unhide))}


def step(s, q, steps):
    for _ in range(3):
        s.search_vectors(None, 10, q)
    wall, dev, coarse = [], [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        s.search_vectors(None, 10, q)
        wall.append((time.perf_counter() - t0) * 1e3)
        st = s.last_stats()
        dev.append(st["total_ms"])
        coarse.append(st["coarse_survivors"])
    return {"wall_ms": float(np.median(wall)), "total_ms": float(np.median(dev)), "coarse_survivors": int(np.median(coarse))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--explicit-rows", type=int, default=10_000_000)
    ap.add_argument("--synthetic-rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    ctx = pa.Context(0)
    rng = np.random.default_rng(1)
    out = {}

    n = a.explicit_rows
    chunk = min(n, 1 << 20)
    rows = rng.standard_normal((chunk, D), dtype=np.float32)
    all_ids = rng.permutation(4 * n).astype(np.int64)[:n]
    s = pa.Searcher(ctx, D, "cosine")
    s.reserve(1, n)
    for r0 in range(0, n, chunk):
        m = min(chunk, n - r0)
        s.add_rows(1, rows[:m], all_ids[r0:r0 + m])
    s.finalize()
    out["explicit"] = {"rows": n, "runs": [latency(s, lambda c, g: g.choice(all_ids, c, replace=False), c, rng) for c in (1, 1000, 100_000)]}
    s.close()
    del rows

    n = a.synthetic_rows
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, n, 0x5EED)
    s.finalize()
    out["synthetic"] = {"rows": n, "runs": [latency(s, lambda c, g: g.choice(n, c, replace=False), c, rng) for c in (1, 1000, 100_000)]}
    q = rng.standard_normal((64, D), dtype=np.float32)
    before = step(s, q, a.steps)
    hidden = rng.choice(n, n // 100, replace=False)
    t0 = time.perf_counter()
    s.hide_items(hidden)
    hide_ms = (time.perf_counter() - t0) * 1e3
    after = step(s, q, a.steps)
    out["step"] = {"rows": n, "B": 64, "k": 10, "hidden": int(hidden.size), "hide_ms": hide_ms, "before": before, "after": after}
    s.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
