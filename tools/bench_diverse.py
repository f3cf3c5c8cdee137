#!/usr/bin/env python3
"""Diverse results (pcv_searcher_search_diverse) beside the passes they are made of: search_vectors with num_results = pool makes
the same ceil(pool / 128) passes without the collect and select steps, so the difference of the two is what the feature costs.

    python tools/bench_diverse.py [--rows 10000000] [--queries 64] [--steps 30] [--warmup 5] [--lam 0.7]
                                  [--settings 10:128,10:1024,128:4096]

A cosine searcher of --rows x 384 synthetic rows under AUTO (the corpus of tools/bench_distinct.py); the queries are stored rows plus
noise.  Per setting k:pool, back to back on the same searcher and in both orders (A B B A), search_diverse(k, lam, pool) and
search_vectors(k = pool): wall ms per call — median, quartiles, min and max over --steps calls after --warmup — and the device time
of the passes inside it (pcv_scan_stats.total_ms, from hipEvents: upload to ranked lists, without the collect and select steps).
The overhead is taken from the wall times: diverse - plain, and as a ratio diverse / plain; it holds the collect kernels, the select
kernel, the allocation of the row scratch where the call gives it back (more than 64 MB), the stream synchronisations and the
download of the result block.  The kernels' own times come from a kernel trace of this script (rocprofv3 --kernel-trace --stats).
Prints one JSON line per setting."""
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
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--settings", default="10:128,10:1024,128:4096")
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    for r0 in range(0, a.rows, SEG):
        s.add_synthetic(1, min(SEG, a.rows - r0), 0x5EED, first_row=r0)
    s.finalize()
    rng = np.random.default_rng(3)
    rows, _ = s.get_rows(rng.integers(0, a.rows, size=a.queries).astype(np.int64))
    q = (rows + 0.05 * rng.standard_normal((a.queries, D))).astype(np.float32)
    for setting in a.settings.split(","):
        k, pool = (int(x) for x in setting.split(":"))

        def diverse():
            return s.search_diverse(None, k, q, a.lam, pool=pool)

        def plain():
            return s.search_vectors(None, pool, q)

        got = diverse()
        launches = s.last_stats()["scan_launches"]
        full = plain()
        assert (got[4] == k).all() and (got[5] == min(pool, a.rows)).all()
        assert (got[0][:, 0] == full[0][:, 0]).all()  # the first pick is the head of the list
        rank_of = np.take_along_axis(full[0], got[3].astype(np.int64), axis=1)
        assert (rank_of == got[0]).all()  # every pick sits in the plain list at its rank
        d1 = timed(diverse, s, a.warmup, a.steps)
        p1 = timed(plain, s, a.warmup, a.steps)
        p2 = timed(plain, s, a.warmup, a.steps)
        d2 = timed(diverse, s, a.warmup, a.steps)
        dw, pw = np.concatenate([d1[0], d2[0]]), np.concatenate([p1[0], p2[0]])
        dd, pd = np.concatenate([d1[1], d2[1]]), np.concatenate([p1[1], p2[1]])
        over = float(np.median(dw) - np.median(pw))
        print(json.dumps({
            "metric": "search_diverse vs search_vectors(k=%d) (ms per call)" % pool, "rows": s.num_rows, "dim": D, "queries": a.queries,
            "k": k, "lambda": a.lam, "pool": pool, "diverse_launches": launches,
            "diverse_wall_ms": spread(dw), "plain_wall_ms": spread(pw),
            "diverse_pass_device_ms": spread(dd), "plain_pass_device_ms": spread(pd),
            "overhead_wall_ms": over, "overhead_ratio": float(np.median(dw) / np.median(pw)),
            "one_pass_device_ms": float(np.median(dd)) / max(launches, 1),
            "median_by_order_wall_ms": {"diverse": [float(np.median(d1[0])), float(np.median(d2[0]))],
                                        "plain": [float(np.median(p1[0])), float(np.median(p2[0]))]},
            "last_rank_median": float(np.median(got[3].max(axis=1))), "exact_share": float(got[6].mean()),
            "screen_bits": s.last_stats()["screen_bits"],
        }), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
