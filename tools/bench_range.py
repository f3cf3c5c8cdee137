#!/usr/bin/env python3
"""Range search (pcv_searcher_search_range) against the two things it stands between: a top-10 search (one pass: the floor) and
search_vectors with num_results = the largest match count (the only way without it: ceil(H / 128) passes).

    python tools/bench_range.py [--rows 10000000] [--queries 16] [--steps 20] [--warmup 5] [--matches 10,1000,20000]

A cosine searcher of --rows x 384 synthetic rows under AUTO; the queries are stored rows plus noise.  For each target in --matches
the bounds are taken from a prior top-k search so that every query has about that many matches.  Times, back to back on the same
searcher and in both orders, search_range, search_vectors(k = 10) and search_vectors(k = largest count): wall ms per call (median)
and the device time inside it (pcv_scan_stats.total_ms), plus what the survivors of the fixed thresholds were: listed rows,
coarse survivors (each one f32-row read, or one mid-copy row where a mid copy exists) and launches.  Prints one JSON line per
target."""
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
SEG = 2_500_000  # rows per synthetic segment


def timed(fn, s, warmup, steps):
    for _ in range(warmup):
        fn()
    wall, dev = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(s.last_stats()["total_ms"])
    return float(np.median(wall)), float(np.median(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--matches", default="10,1000,20000")
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    for r0 in range(0, a.rows, SEG):
        s.add_synthetic(1, min(SEG, a.rows - r0), 0x5EED, first_row=r0)
    s.finalize()
    rng = np.random.default_rng(3)
    rows, _ = s.get_rows(rng.integers(0, a.rows, size=a.queries).astype(np.int64))
    q = (rows + 0.05 * rng.standard_normal((a.queries, D))).astype(np.float32)
    for target in [int(x) for x in a.matches.split(",")]:
        full = s.search_vectors(None, target, q)
        bounds = np.ascontiguousarray(full[1][:, target - 1])
        got = s.search_range(None, bounds, q, 2 * target + 16)
        st = s.last_stats()
        counts = got[2]
        assert (counts >= target).all() and not got[3].any() and (got[0][:, :target] == full[0]).all()
        H = int(counts.max())

        def range_call():
            s.search_range(None, bounds, q, H)

        def top10():
            s.search_vectors(None, 10, q)

        def paged():
            s.search_vectors(None, H, q)

        r1 = timed(range_call, s, a.warmup, a.steps)
        t1 = timed(top10, s, a.warmup, a.steps)
        p1 = timed(paged, s, min(a.warmup, 2), max(3, a.steps // 4) if H > 1024 else a.steps)
        paged_launches = s.last_stats()["scan_launches"]
        p2 = timed(paged, s, 0, max(3, a.steps // 4) if H > 1024 else a.steps)
        t2 = timed(top10, s, a.warmup, a.steps)
        r2 = timed(range_call, s, a.warmup, a.steps)
        rs = s.last_stats()
        print(json.dumps({
            "metric": "search_range vs search_vectors (ms per call, median; [first order, second order])", "rows": s.num_rows, "dim": D,
            "queries": a.queries, "target_matches": target, "median_matches": float(np.median(counts)), "largest_count": H,
            "search_range_wall_ms": [r1[0], r2[0]], "search_range_device_ms": [r1[1], r2[1]],
            "top10_wall_ms": [t1[0], t2[0]], "top10_device_ms": [t1[1], t2[1]],
            "paged_wall_ms": [p1[0], p2[0]], "paged_device_ms": [p1[1], p2[1]], "paged_launches": paged_launches,
            "range_launches": rs["scan_launches"], "range_first_call_launches": st["scan_launches"],
            "range_listed_rows": rs["candidates"], "range_coarse_survivors": rs["coarse_survivors"],
            "range_mid_survivors": rs["mid_survivors"], "range_scan_ms": rs["scan_ms"], "mid_copy": rs["mid_copy"],
            "screen_bits": rs["screen_bits"],
        }), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
