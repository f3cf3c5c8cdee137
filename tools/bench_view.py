#!/usr/bin/env python3
"""Views (pcv_searcher_create_view): what building one costs, how its searches compare with a searcher built fresh from the
same rows, and whether views change the parent's step.

    python tools/bench_view.py [--explicit-rows 10000000] [--synthetic-rows 100000000] [--steps 20] [--skip-synthetic]

Prints one JSON object:
  explicit   view build for 1e3 / 1e5 / 1e6 / 1e7 allowed ids on a corpus with an id column (add_rows; the rows are copies of
             one 1M-row chunk under distinct ids), int8 copy: wall ms (median of 3), device build_ms of view_stats(), and the
             effective bandwidth of the build: f32 rows read + written (the copies come on top), over the device time
  synthetic  the same on synthetic rows (implicit ids: the rows are found by arithmetic on the host)
  search     the 64-query top-10 step of the 1e6-id view next to a searcher built fresh from the same rows (wall ms, median of
             --steps; device total_ms; results compared bit for bit)
  parent     the parent's 64-query top-10 step before any view exists and while four views of it are alive
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
SIZES = (1_000, 100_000, 1_000_000, 10_000_000)


def step(s, q, steps):
    for _ in range(3):
        s.search_vectors(None, 10, q)
    wall, dev = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        res = s.search_vectors(None, 10, q)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(s.last_stats()["total_ms"])
    return {"wall_ms": float(np.median(wall)), "total_ms": float(np.median(dev))}, res


def builds(s, pick, n, reps=3):
    wall, dev = [], []
    for r in range(reps):
        ids = pick(n, r)
        t0 = time.perf_counter()
        v = s.view(ids)
        wall.append((time.perf_counter() - t0) * 1e3)
        st = v.view_stats()
        dev.append(st["build_ms"])
        rows = st["rows"]
        v.close()
    ms = float(np.median(dev))
    moved = 2.0 * rows * D * 4  # f32 pieces read from the parent and written to the view
    return {"ids": n, "rows": rows, "wall_ms": float(np.median(wall)), "build_ms": ms, "f32_rw_GBps": moved / (ms * 1e6) if ms > 0 else None}


def fill(s, source, rows, all_ids):
    n, chunk = all_ids.size, rows.shape[0]
    s.reserve(source, n)
    for r0 in range(0, n, chunk):
        m = min(chunk, n - r0)
        s.add_rows(source, rows[:m], all_ids[r0:r0 + m])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--explicit-rows", type=int, default=10_000_000)
    ap.add_argument("--synthetic-rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-synthetic", action="store_true")
    a = ap.parse_args()
    ctx = pa.Context(0)
    rng = np.random.default_rng(1)
    out = {}

    n = a.explicit_rows
    chunk = min(n, 1 << 20)
    rows = rng.standard_normal((chunk, D), dtype=np.float32)
    all_ids = rng.permutation(4 * n).astype(np.int64)[:n]
    s = pa.Searcher(ctx, D, "cosine")
    s.set_screening_copy("int8")
    fill(s, 1, rows, all_ids)
    s.finalize()
    q = rng.standard_normal((64, D), dtype=np.float32)
    before, _ = step(s, q, a.steps)
    out["explicit"] = [builds(s, lambda c, r: np.random.default_rng(r).choice(all_ids, min(c, n), replace=False), c) for c in SIZES]
    # a 1e6-id view against a searcher built fresh from the same rows (row i of the corpus is rows[i % chunk])
    allow = np.random.default_rng(7).choice(all_ids, min(n, 1_000_000), replace=False)
    v = s.view(allow)
    at = np.flatnonzero(np.isin(all_ids, allow))
    f = pa.Searcher(ctx, D, "cosine")
    f.set_screening_copy("int8")
    f.reserve(1, at.size)
    for p0 in range(0, at.size, 1 << 18):
        sl = at[p0:p0 + (1 << 18)]
        f.add_rows(1, rows[sl % chunk], all_ids[sl])
    f.finalize()
    vs, vres = step(v, q, a.steps)
    fs, fres = step(f, q, a.steps)
    same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(vres, fres))
    out["search"] = {"rows": int(at.size), "B": 64, "k": 10, "view": vs, "fresh": fs, "identical": bool(same)}
    f.close()
    views = [v] + [s.view(np.random.default_rng(20 + i).choice(all_ids, 100_000, replace=False)) for i in range(3)]
    after, _ = step(s, q, a.steps)
    out["parent"] = {"rows": n, "B": 64, "k": 10, "before": before, "with_4_views": after}
    for x in views:
        x.close()
    s.close()
    del rows

    if not a.skip_synthetic:
        n = a.synthetic_rows
        s = pa.Searcher(ctx, D, "cosine")
        s.set_screening_copy("int8")
        s.add_synthetic(1, n, 0x5EED)
        s.finalize()
        out["synthetic"] = [builds(s, lambda c, r: np.random.default_rng(r).choice(n, c, replace=False), c) for c in SIZES]
        s.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
