#!/usr/bin/env python3
"""Boosted search (pcv_searcher_search_boosted) beside what it is made of.

    python tools/bench_boost.py [--rows 10000000] [--queries 64] [--steps 30] [--warmup 5] [--k 10] [--pool 128]

A cosine searcher of --rows x 384 synthetic rows under AUTO (item id = row number, no id column) with the value permutation of
tools/bench_where.py: the value of an id is id * 2654435761 mod --rows; the queries are stored rows plus noise.

(1) Three calls on the same searcher in the same run, in the order A B C C B A, --steps calls each time after --warmup:
      a  search_boosted(k, pool) with a zero boost — one pass and the boosted select step;
      b  search_where(k, pool) under a predicate every row passes — one pass and the filtered select step;
      c  search_vectors(k = min(pool, 128)) — the same pass alone.
    Wall ms per call: median, quartiles, min and max.  a - c and b - c are the two select steps' costs (kernel, stream
    synchronisation, download of the kept rows); the question is whether they are the same fixed cost.
(2) How many entries a recency-like boost needs before the certificate holds: knots at 0, 1/4, 1/2, 3/4 and the end of the value
    range with boosts 0, w/8, w/4, w/2, w for w = 0.05, 0.2 and 1.0, k results, pool 4096 — examined entries per query (quartiles)
    and how many queries were certified.
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
MUL = 2654435761  # a prime: id -> id * MUL mod rows is a permutation for every rows below it


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return np.array(wall)


def spread(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "q1": float(np.percentile(x, 25)), "q3": float(np.percentile(x, 75)),
            "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--pool", type=int, default=128)
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    for r0 in range(0, a.rows, SEG):
        s.add_synthetic(1, min(SEG, a.rows - r0), 0x5EED, first_row=r0)
    s.finalize()
    ids = np.arange(a.rows, dtype=np.int64)
    assert a.rows < MUL
    s.set_values(ids, (ids * MUL) % a.rows)
    rng = np.random.default_rng(3)
    rows, _ = s.get_rows(rng.integers(0, a.rows, size=a.queries).astype(np.int64))
    q = (rows + 0.05 * rng.standard_normal((a.queries, D))).astype(np.float32)
    plain_k = min(a.pool, 128)

    def boosted():
        return s.search_boosted(None, a.k, q, [0], [0.0], 0.0, a.pool)

    def where():
        return s.search_where(None, a.k, q, 0, a.rows - 1, pool=a.pool)

    def plain():
        return s.search_vectors(None, plain_k, q)

    got = boosted()
    launches = s.last_stats()["scan_launches"]
    full = plain()
    assert (got[0] == full[0][:, : a.k]).all() and (got[1].view(np.uint32) == full[1][:, : a.k].view(np.uint32)).all()
    assert (got[3] == (got[0] * MUL) % a.rows).all() and (got[6] == plain_k).all() and got[7].all()
    assert (where()[0] == got[0]).all()
    # ---- (1) A B C C B A ----
    a1 = timed(boosted, a.warmup, a.steps)
    b1 = timed(where, a.warmup, a.steps)
    c1 = timed(plain, a.warmup, a.steps)
    c2 = timed(plain, a.warmup, a.steps)
    b2 = timed(where, a.warmup, a.steps)
    a2 = timed(boosted, a.warmup, a.steps)
    aw, bw, cw = np.concatenate([a1, a2]), np.concatenate([b1, b2]), np.concatenate([c1, c2])
    # ---- (2) entries before the certificate holds ----
    knots = [0, a.rows // 4, a.rows // 2, 3 * (a.rows // 4), a.rows - 1]
    need = {}
    for w in (0.05, 0.2, 1.0):
        r = s.search_boosted(None, a.k, q, knots, [0.0, w / 8, w / 4, w / 2, w], 0.0, 4096)
        need[str(w)] = {"examined": spread(r[6]), "certified": int(r[7].sum()), "queries": a.queries}
    print(json.dumps({
        "metric": "search_boosted (zero boost) vs search_where (everything passes) vs search_vectors(k=%d) (wall ms per call)" % plain_k,
        "rows": s.num_rows, "dim": D, "queries": a.queries, "k": a.k, "pool": a.pool, "boosted_launches": launches,
        "boosted_wall_ms": spread(aw), "where_wall_ms": spread(bw), "plain_wall_ms": spread(cw),
        "boosted_select_step_ms": float(np.median(aw) - np.median(cw)), "where_select_step_ms": float(np.median(bw) - np.median(cw)),
        "median_by_order_wall_ms": {"boosted": [float(np.median(a1)), float(np.median(a2))], "where": [float(np.median(b1)), float(np.median(b2))],
                                    "plain": [float(np.median(c1)), float(np.median(c2))]},
        "screen_bits": s.last_stats()["screen_bits"], "entries_until_certified": need,
        "date": time.strftime("%Y-%m-%d"),
    }), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
