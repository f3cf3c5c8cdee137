#!/usr/bin/env python3
"""Search by example (pcv_searcher_search_like): what the id lookup, the query build and the extra rank cost on top of a search
with the same vectors held on the host.

    python tools/bench_like.py [--rows 10000000] [--queries 64] [--steps 20] [--warmup 5] [--implicit]

A searcher of --rows x 384 rows added with explicit ids (`add_rows`: one random chunk of at most 2^20 rows, rotated by one feature
per repeat so that no two rows are equal, under permuted ids; the lookup streams the 8 B per row id column), or --implicit
(synthetic rows, ids by arithmetic, nothing streamed).  Times, back to back on the same searcher, `search_like` with --queries
single examples, k = 10, exclusion on, and `search_vectors` with the same vectors on the host, k = 10, in both orders.  Prints
one JSON line: both medians and their difference (wall ms), the device time of the search inside each, and `like_queries`
alone."""
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
SEG = 2_500_000  # rows per synthetic segment (--implicit)


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
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--implicit", action="store_true", help="keep the implicit ids (no id column to stream)")
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    rng = np.random.default_rng(3)
    if a.implicit:
        for r0 in range(0, a.rows, SEG):
            s.add_synthetic(1, min(SEG, a.rows - r0), 0x5EED, first_row=r0)
        all_ids = np.arange(a.rows, dtype=np.int64)
    else:
        chunk = min(a.rows, 1 << 20)
        rows = rng.standard_normal((chunk, D), dtype=np.float32)
        all_ids = rng.permutation(4 * a.rows).astype(np.int64)[:a.rows]
        s.reserve(1, a.rows)
        for i, r0 in enumerate(range(0, a.rows, chunk)):
            m = min(chunk, a.rows - r0)
            s.add_rows(1, np.roll(rows[:m], i, axis=1), all_ids[r0:r0 + m])
        del rows
    s.finalize()
    pick = rng.choice(all_ids, a.queries, replace=False)
    groups = [[int(x)] for x in pick]
    v, found, members = s.like_queries(groups)
    assert found.all() and (members == 1).all()
    k = 10
    like = s.search_like(None, k, groups, exclude_examples=True)
    plain = s.search_vectors(None, k + 1, v)
    assert (plain[0][:, 0] == pick).all() and (like[0] == plain[0][:, 1:]).all()
    # back to back, the same build and searcher; twice, in both orders
    t_like, d_like = timed(lambda: s.search_like(None, k, groups, exclude_examples=True), s, a.warmup, a.steps)
    t_vec, d_vec = timed(lambda: s.search_vectors(None, k, v), s, a.warmup, a.steps)
    t_vec2, d_vec2 = timed(lambda: s.search_vectors(None, k, v), s, a.warmup, a.steps)
    t_like2, d_like2 = timed(lambda: s.search_like(None, k, groups, exclude_examples=True), s, a.warmup, a.steps)
    t_build, _ = timed(lambda: s.like_queries(groups), s, a.warmup, a.steps)
    print(json.dumps({
        "metric": "search_like vs search_vectors (wall ms per call, median)", "rows": s.num_rows, "dim": D, "queries": a.queries, "k": k,
        "ids": "implicit" if a.implicit else "explicit", "segments": s.num_segments,
        "search_like_ms": [t_like, t_like2], "search_vectors_ms": [t_vec, t_vec2],
        "difference_ms": [t_like - t_vec, t_like2 - t_vec2], "like_queries_ms": t_build,
        "device_total_ms": {"search_like": [d_like, d_like2], "search_vectors": [d_vec, d_vec2]},
        "id_column_bytes": 0 if a.implicit else 8 * s.num_rows,
    }))
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
