#!/usr/bin/env python3
"""Distinct results (pcv_searcher_search_distinct) beside the pass they are made of: search_vectors with num_results = 128 is the
same single pass without the select step, so the difference of the two is what the feature costs.

    python tools/bench_distinct.py [--rows 10000000] [--queries 64] [--steps 30] [--warmup 5] [--k 10] [--threshold 0.95] [--pool 128]

A cosine searcher of --rows x 384 synthetic rows under AUTO; the queries are stored rows plus noise.  Times, back to back on the
same searcher and in both orders (A B B A), search_distinct(k, threshold, pool) and search_vectors(k = min(pool, 128)): wall ms per
call — median, quartiles, min and max over --steps calls after --warmup — and the device time of the passes inside it
(pcv_scan_stats.total_ms: upload to ranked lists, without the select step).  The select step's share is taken from the wall
times: (distinct - plain) / distinct; it holds the select kernel, its stream synchronisation and the download of the kept rows.
Prints one JSON line."""
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
    return np.array(wall), np.array(dev)


def spread(x):
    return {"median": float(np.median(x)), "q1": float(np.percentile(x, 25)), "q3": float(np.percentile(x, 75)),
            "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--threshold", type=float, default=0.95)
    ap.add_argument("--pool", type=int, default=128)
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    for r0 in range(0, a.rows, SEG):
        s.add_synthetic(1, min(SEG, a.rows - r0), 0x5EED, first_row=r0)
    s.finalize()
    rng = np.random.default_rng(3)
    rows, _ = s.get_rows(rng.integers(0, a.rows, size=a.queries).astype(np.int64))
    q = (rows + 0.05 * rng.standard_normal((a.queries, D))).astype(np.float32)
    plain_k = min(a.pool, 128)

    def distinct():
        return s.search_distinct(None, a.k, q, a.threshold, pool=a.pool)

    def plain():
        return s.search_vectors(None, plain_k, q)

    got = distinct()
    launches = s.last_stats()["scan_launches"]
    full = plain()
    assert (got[2] == a.k).all() and (got[0] == full[0][:, : a.k]).all()  # synthetic rows have no near-duplicates: the plain top-k
    d1 = timed(distinct, s, a.warmup, a.steps)
    p1 = timed(plain, s, a.warmup, a.steps)
    p2 = timed(plain, s, a.warmup, a.steps)
    d2 = timed(distinct, s, a.warmup, a.steps)
    dw, pw = np.concatenate([d1[0], d2[0]]), np.concatenate([p1[0], p2[0]])
    dd, pd = np.concatenate([d1[1], d2[1]]), np.concatenate([p1[1], p2[1]])
    select_ms = float(np.median(dw) - np.median(pw))
    print(json.dumps({
        "metric": "search_distinct vs search_vectors(k=%d) (ms per call)" % plain_k, "rows": s.num_rows, "dim": D, "queries": a.queries,
        "k": a.k, "threshold": a.threshold, "pool": a.pool, "distinct_launches": launches,
        "distinct_wall_ms": spread(dw), "plain_wall_ms": spread(pw),
        "distinct_pass_device_ms": spread(dd), "plain_pass_device_ms": spread(pd),
        "select_step_wall_ms": select_ms, "select_step_share": select_ms / float(np.median(dw)),
        "median_by_order_wall_ms": {"distinct": [float(np.median(d1[0])), float(np.median(d2[0]))],
                                    "plain": [float(np.median(p1[0])), float(np.median(p2[0]))]},
        "examined_median": float(np.median(got[4])), "screen_bits": s.last_stats()["screen_bits"],
    }), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
