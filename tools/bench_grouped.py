#!/usr/bin/env python3
"""Grouped results (pcv_searcher_search_grouped) beside the pass they are made of, and the group table's upsert.

    python tools/bench_grouped.py [--rows 10000000] [--queries 64] [--steps 30] [--warmup 5] [--k 10] [--pool 128] [--group-size 8]

A cosine searcher of --rows x 384 synthetic rows under AUTO (item id = row number); the group of an id is id // --group-size; the
queries are stored rows plus noise.

1. search_grouped(k, pool) and search_vectors(k = min(pool, 128)) — the same single pass without the select step — back to back on
   the same searcher and in both orders (A B B A): wall ms per call, median, quartiles, min and max over --steps calls after
   --warmup, and the device time of the passes inside it (pcv_scan_stats.total_ms: upload to ranked lists, without the select
   step).  The select step's share is taken from the wall times: (grouped - plain) / grouped; it holds the select kernel, its
   stream synchronisation and the download of the kept rows.
2. set_groups for all --rows ids in one batch on an empty table (last_set_ms of pcv_group_stats: upload, growth and the two upsert
   launches per 2^22 ids; ids per second), then a second batch of as many new ids, which forces a rehash of the full
   table (slots < 4 * rows before it, 4 * rows needed).
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
    ap.add_argument("--pool", type=int, default=128)
    ap.add_argument("--group-size", type=int, default=8)
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    for r0 in range(0, a.rows, SEG):
        s.add_synthetic(1, min(SEG, a.rows - r0), 0x5EED, first_row=r0)
    s.finalize()
    # ---- 2. the table (first: the searches below need it) ----
    ids = np.arange(a.rows, dtype=np.int64)
    t0 = time.perf_counter()
    s.set_groups(ids, ids // a.group_size)
    first_wall = (time.perf_counter() - t0) * 1e3
    first = s.group_stats()
    assert first["ids"] == a.rows and first["entries"] == a.rows
    more_ids = np.arange(a.rows, 2 * a.rows, dtype=np.int64)  # ids no row carries: the searches do not see them
    t0 = time.perf_counter()
    s.set_groups(more_ids, more_ids // a.group_size)
    second_wall = (time.perf_counter() - t0) * 1e3
    second = s.group_stats()
    assert second["rehashes"] == first["rehashes"] + 1 and second["entries"] == a.rows + len(more_ids)
    # ---- 1. the search ----
    rng = np.random.default_rng(3)
    rows, _ = s.get_rows(rng.integers(0, a.rows, size=a.queries).astype(np.int64))
    q = (rows + 0.05 * rng.standard_normal((a.queries, D))).astype(np.float32)
    plain_k = min(a.pool, 128)

    def grouped():
        return s.search_grouped(None, a.k, q, pool=a.pool)

    def plain():
        return s.search_vectors(None, plain_k, q)

    got = grouped()
    launches = s.last_stats()["scan_launches"]
    full = plain()
    for b in range(a.queries):  # the kept rows are the first of each group in the plain list
        seen, want = set(), []
        for i in full[0][b].tolist():
            if i // a.group_size not in seen:
                seen.add(i // a.group_size)
                want.append(i)
        n = min(a.k, len(want))
        assert got[0][b, :n].tolist() == want[:n], b
    g1 = timed(grouped, s, a.warmup, a.steps)
    p1 = timed(plain, s, a.warmup, a.steps)
    p2 = timed(plain, s, a.warmup, a.steps)
    g2 = timed(grouped, s, a.warmup, a.steps)
    gw, pw = np.concatenate([g1[0], g2[0]]), np.concatenate([p1[0], p2[0]])
    gd, pd = np.concatenate([g1[1], g2[1]]), np.concatenate([p1[1], p2[1]])
    select_ms = float(np.median(gw) - np.median(pw))
    print(json.dumps({
        "metric": "search_grouped vs search_vectors(k=%d) (ms per call)" % plain_k, "rows": s.num_rows, "dim": D, "queries": a.queries,
        "k": a.k, "pool": a.pool, "group_size": a.group_size, "grouped_launches": launches,
        "grouped_wall_ms": spread(gw), "plain_wall_ms": spread(pw),
        "grouped_pass_device_ms": spread(gd), "plain_pass_device_ms": spread(pd),
        "select_step_wall_ms": select_ms, "select_step_share": select_ms / float(np.median(gw)),
        "median_by_order_wall_ms": {"grouped": [float(np.median(g1[0])), float(np.median(g2[0]))],
                                    "plain": [float(np.median(p1[0])), float(np.median(p2[0]))]},
        "examined_median": float(np.median(got[5])), "collapsed_total": int(got[4].sum()), "screen_bits": s.last_stats()["screen_bits"],
        "set_groups_first": {"ids": a.rows, "last_set_ms": first["last_set_ms"], "wall_ms": first_wall, "slots": first["slots"],
                             "ids_per_s": a.rows / (first["last_set_ms"] * 1e-3)},
        "set_groups_rehash": {"ids": len(more_ids), "last_set_ms": second["last_set_ms"], "wall_ms": second_wall, "slots": second["slots"],
                              "rehashes": second["rehashes"], "ids_per_s": len(more_ids) / (second["last_set_ms"] * 1e-3)},
    }), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
