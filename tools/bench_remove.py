#!/usr/bin/env python3
"""Removed items (pcv_searcher_remove_ids): what dropping rows in place costs, next to the only way the library had before —
uploading the remaining rows of the source again (staging source + pcv_searcher_replace_source) — and what a search step
costs afterwards, next to a searcher built fresh from the remaining rows and next to the same rows hidden with hide_ids.

    python tools/bench_remove.py [--explicit-rows 10000000] [--synthetic-rows 100000000] [--steps 20] [--skip-synthetic]
                                 [--only remove|reupload|search]

Prints one JSON object:
  explicit   remove_ids of 1e3 / 1e5 / 1e6 / 1e7 random ids, one after the other on the same searcher (rows_before says what
             was left), on a corpus with an id column (the rows are copies of one 1M-row chunk under distinct ids), int8 copy:
             wall ms of the call (it ends with a stream synchronise, so it covers the device time), rows removed, and the f32
             traffic of the moved rows (read twice, written twice) over that time
  synthetic  the same on synthetic rows (implicit ids: the first removal also writes the segment's id column)
  reupload   the same 1e3 / 1e5 / 1e6-id removals done by uploading the remaining rows from host memory into the staging
             source, replace_source, finalize (wall ms)
  search     the 64-query top-10 step after removing 30 % of the rows, beside a searcher built fresh from the remaining rows
             (five timings of it give the spread) and beside the full searcher with the same 30 % hidden; results compared
The kernel split (mark, move, re-pack) comes from a run under a kernel-trace profiler of `--only remove`.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import perceive_amd as pa  # noqa: E402
from perceive_amd import _ffi  # noqa: E402
from perceive_amd.search import STAGING_SOURCE  # noqa: E402

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


def fill(s, source, rows, all_ids):
    n, chunk = all_ids.size, rows.shape[0]
    s.reserve(source, n)
    for r0 in range(0, n, chunk):
        m = min(chunk, n - r0)
        s.add_rows(source, rows[:m], all_ids[r0:r0 + m])


def removals(ctx, s, live_ids):
    """Remove 1e3, 1e5, ... random ids of `live_ids` (ascending positions = row order), one call each."""
    out = []
    for i, c in enumerate(SIZES):
        before = live_ids.size
        if before == 0:
            break
        at = np.sort(np.random.default_rng(i).choice(before, min(c, before), replace=False))
        ids = live_ids[at]
        ctx.synchronize()
        t0 = time.perf_counter()
        removed = s.remove_items(ids)
        ms = (time.perf_counter() - t0) * 1e3
        moved = before - int(at[0]) - removed  # rows behind the first removed one that stay
        out.append({"ids": int(ids.size), "rows_before": int(before), "removed": int(removed), "wall_ms": ms,
                    "moved_rows": int(moved), "f32_traffic_GBps": 4.0 * moved * D * 4 / (ms * 1e6)})
        keep = np.ones(before, bool)
        keep[at] = False
        live_ids = live_ids[keep]
    return out


def reupload(ctx, s, rows, live_ids, chunk):
    """The same removals the way they were done before: the remaining rows go up again (row i of the corpus is rows[i % chunk])."""
    out = []
    live_at = np.arange(live_ids.size)
    for i, c in enumerate(SIZES[:3]):
        before = live_ids.size
        at = np.sort(np.random.default_rng(i).choice(before, min(c, before), replace=False))
        keep = np.ones(before, bool)
        keep[at] = False
        live_ids, live_at = live_ids[keep], live_at[keep]
        ctx.synchronize()
        t0 = time.perf_counter()
        s.reserve(STAGING_SOURCE, live_ids.size)
        for p0 in range(0, live_ids.size, 1 << 18):
            sl = slice(p0, p0 + (1 << 18))
            s.add_rows(STAGING_SOURCE, rows[live_at[sl] % chunk], live_ids[sl])
        _ffi.check(_ffi.lib().pcv_searcher_replace_source(s._handle, C.c_int64(STAGING_SOURCE), C.c_int64(1)))
        s.finalize()
        ms = (time.perf_counter() - t0) * 1e3
        out.append({"ids": int(at.size), "rows_before": int(before), "wall_ms": ms})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--explicit-rows", type=int, default=10_000_000)
    ap.add_argument("--synthetic-rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-synthetic", action="store_true")
    ap.add_argument("--only", choices=["remove", "reupload", "search"])
    a = ap.parse_args()
    ctx = pa.Context(0)
    rng = np.random.default_rng(1)
    out = {}
    n = a.explicit_rows
    chunk = min(n, 1 << 20)
    rows = rng.standard_normal((chunk, D), dtype=np.float32)
    all_ids = rng.permutation(4 * n).astype(np.int64)[:n]
    q = rng.standard_normal((64, D), dtype=np.float32)

    def build(ids_at=None):
        s = pa.Searcher(ctx, D, "cosine")
        s.set_screening_copy("int8")
        if ids_at is None:
            fill(s, 1, rows, all_ids)
        else:
            s.reserve(1, ids_at.size)
            for p0 in range(0, ids_at.size, 1 << 18):
                sl = ids_at[p0:p0 + (1 << 18)]
                s.add_rows(1, rows[sl % chunk], all_ids[sl])
        s.finalize()
        return s

    if a.only in (None, "remove"):
        s = build()
        out["explicit"] = removals(ctx, s, all_ids)
        s.close()
    if a.only in (None, "reupload"):
        s = build()
        out["reupload"] = reupload(ctx, s, rows, all_ids, chunk)
        s.close()
    if a.only in (None, "search"):
        gone_at = np.sort(np.random.default_rng(30).choice(n, n * 3 // 10, replace=False))
        keep_at = np.setdiff1d(np.arange(n), gone_at)
        s = build()
        s.remove_items(all_ids[gone_at])
        removed, rres = step(s, q, a.steps)
        s.close()
        f = build(keep_at)
        runs = [step(f, q, a.steps) for _ in range(5)]
        fres = runs[0][1]
        f.close()
        h = build()
        h.hide_items(all_ids[gone_at])
        hidden, hres = step(h, q, a.steps)
        h.close()
        same = lambda x, y: all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(x, y))  # noqa: E731
        out["search"] = {"rows": n, "removed": int(gone_at.size), "B": 64, "k": 10, "after_remove": removed,
                         "fresh": [r[0] for r in runs], "hidden_instead": hidden,
                         "identical_to_fresh": bool(same(rres, fres)), "hidden_identical": bool(same(hres, fres))}
    del rows
    if not a.skip_synthetic and a.only in (None, "remove"):
        n = a.synthetic_rows
        s = pa.Searcher(ctx, D, "cosine")
        s.set_screening_copy("int8")
        s.add_synthetic(1, n, 0x5EED)
        s.finalize()
        out["synthetic"] = removals(ctx, s, np.arange(n, dtype=np.int64))
        s.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
