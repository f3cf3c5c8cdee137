#!/usr/bin/env python3
"""Item values and filtered search (pcv_searcher_set_values / _count_where / _search_where / _create_view_where) beside what they are
made of.

    python tools/bench_where.py [--rows 10000000] [--queries 64] [--steps 30] [--warmup 5] [--k 10] [--pool 128]

A cosine searcher of --rows x 384 synthetic rows under AUTO (item id = row number, no id column); the value of an id is
id * 2654435761 mod --rows — a permutation of 0 .. rows - 1, so `value < n` passes exactly n rows, scattered over the corpus; the
queries are stored rows plus noise.

(a) search_where(k, pool) under a predicate every row passes and search_vectors(k = min(pool, 128)) — the same single pass without the
    select step — back to back on the same searcher and in both orders (A B B A): wall ms per call, median, quartiles, min and max
    over --steps calls after --warmup, and the device time of the passes inside.  The select step's cost is the difference of the
    wall medians: the select kernel, its stream synchronisation and the download of the kept rows.
(b) count_where over all rows with the table at --rows entries: wall ms per call, at three pass rates.
(c) create_view_where at 1e3, 1e5, 1e6 and 1e7 passing rows (those that fit --rows) beside create_view over the same ids: wall ms of
    the call and the device time of the copy (view_stats build_ms); for the id-list view the wall time includes sorting the list,
    building and uploading its hash table.
(d) set_values of all --rows ids in one batch on an empty table: last_set_ms of pcv_value_stats and wall ms.
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
    ap.add_argument("--pool", type=int, default=128)
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    for r0 in range(0, a.rows, SEG):
        s.add_synthetic(1, min(SEG, a.rows - r0), 0x5EED, first_row=r0)
    s.finalize()
    # ---- (d) the table (first: everything below needs it) ----
    ids = np.arange(a.rows, dtype=np.int64)
    values = (ids * MUL) % a.rows
    assert a.rows < MUL
    t0 = time.perf_counter()
    s.set_values(ids, values)
    set_wall = (time.perf_counter() - t0) * 1e3
    table = s.value_stats()
    assert table["ids"] == a.rows and table["entries"] == a.rows
    every = (0, a.rows - 1)
    # ---- (a) the select step ----
    rng = np.random.default_rng(3)
    rows, _ = s.get_rows(rng.integers(0, a.rows, size=a.queries).astype(np.int64))
    q = (rows + 0.05 * rng.standard_normal((a.queries, D))).astype(np.float32)
    plain_k = min(a.pool, 128)

    def where():
        return s.search_where(None, a.k, q, *every, pool=a.pool)

    def plain():
        return s.search_vectors(None, plain_k, q)

    got = where()
    launches = s.last_stats()["scan_launches"]
    full = plain()
    assert (got[0] == full[0][:, : a.k]).all() and (got[2] == (got[0] * MUL) % a.rows).all() and (got[4] == a.k).all()
    w1 = timed(where, s, a.warmup, a.steps)
    p1 = timed(plain, s, a.warmup, a.steps)
    p2 = timed(plain, s, a.warmup, a.steps)
    w2 = timed(where, s, a.warmup, a.steps)
    ww, pw = np.concatenate([w1[0], w2[0]]), np.concatenate([p1[0], p2[0]])
    wd, pd = np.concatenate([w1[1], w2[1]]), np.concatenate([p1[1], p2[1]])
    select_ms = float(np.median(ww) - np.median(pw))
    # ---- (b) the count ----
    counts = {}
    for n in sorted({a.rows, a.rows // 2, max(1, a.rows // 1000)}):
        assert s.count_where(None, 0, n - 1) == (n, n)
        wall = []
        for i in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            s.count_where(None, 0, n - 1)
            if i >= a.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
        counts[str(n)] = spread(np.array(wall))
    # ---- (c) the views ----
    views = {}
    for n in (1_000, 100_000, 1_000_000, 10_000_000):
        if n > a.rows:
            continue
        t0 = time.perf_counter()
        v = s.view_where(0, n - 1)
        where_wall = (time.perf_counter() - t0) * 1e3
        where_st = v.view_stats()
        assert where_st["rows"] == n
        allow = ids[values < n]
        t0 = time.perf_counter()
        w = s.view(allow)
        list_wall = (time.perf_counter() - t0) * 1e3
        list_st = w.view_stats()
        assert list_st["rows"] == n
        a_ids, a_sc, _ = v.search_vectors(None, a.k, q)
        b_ids, b_sc, _ = w.search_vectors(None, a.k, q)
        assert (a_ids == b_ids).all() and (a_sc.view(np.uint32) == b_sc.view(np.uint32)).all()
        views[str(n)] = {"view_where_wall_ms": where_wall, "view_where_build_ms": where_st["build_ms"],
                         "view_ids_wall_ms": list_wall, "view_ids_build_ms": list_st["build_ms"]}
        v.close()
        w.close()
    print(json.dumps({
        "metric": "search_where (everything passes) vs search_vectors(k=%d) (ms per call)" % plain_k, "rows": s.num_rows, "dim": D,
        "queries": a.queries, "k": a.k, "pool": a.pool, "where_launches": launches,
        "where_wall_ms": spread(ww), "plain_wall_ms": spread(pw), "where_pass_device_ms": spread(wd), "plain_pass_device_ms": spread(pd),
        "select_step_wall_ms": select_ms, "select_step_share": select_ms / float(np.median(ww)),
        "median_by_order_wall_ms": {"where": [float(np.median(w1[0])), float(np.median(w2[0]))],
                                    "plain": [float(np.median(p1[0])), float(np.median(p2[0]))]},
        "screen_bits": s.last_stats()["screen_bits"],
        "count_where_wall_ms": counts, "views": views,
        "set_values": {"ids": a.rows, "last_set_ms": table["last_set_ms"], "wall_ms": set_wall, "slots": table["slots"],
                       "ids_per_s": a.rows / (table["last_set_ms"] * 1e-3)},
    }), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
