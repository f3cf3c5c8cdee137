#!/usr/bin/env python3
"""Updated items (pcv_searcher_update_rows): what updating vectors in place costs, next to rebuilding the source.

    python tools/bench_update.py [--explicit-rows 10000000] [--synthetic-rows 100000000] [--steps 20]

Prints one JSON object:
  explicit   update latency (ms, median of 3) for 1 / 1 000 / 100 000 ids on a corpus with an id column (add_rows; the rows are
             copies of one 1M-row chunk under distinct ids), with the int8 copy and with the int8 and mid copies
  synthetic  the same on synthetic rows (implicit ids: found by arithmetic on the host)
  rebuild    the same explicit-id source rebuilt instead: add_rows under the staging id + replace_source + finalize (ms)
  step       the 64-query top-10 step on the explicit-id corpus (int8 copy) before and after updating 1 % of its rows: wall ms
             (median of --steps), device total_ms, coarse_survivors of last_stats()
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

D = 384
COPIES = (("int8", "off"), ("int8", "on"))


def latency(s, pick, n, rng, reps=3):
    t = []
    for _ in range(reps):
        ids = pick(n, rng)
        vecs = rng.standard_normal((n, D), dtype=np.float32)
        t0 = time.perf_counter()
        s.update_items(ids, vecs)
        t.append((time.perf_counter() - t0) * 1e3)
    return {"ids": n, "update_ms": float(np.median(t))}


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


def explicit_searcher(ctx, rows, all_ids, screen, mid, source=1):
    s = pa.Searcher(ctx, D, "cosine")
    s.set_screening_copy(screen)
    s.set_mid_copy(mid)
    fill(s, source, rows, all_ids)
    s.finalize()
    return s


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
    a = ap.parse_args()
    ctx = pa.Context(0)
    rng = np.random.default_rng(1)
    out = {"explicit": [], "synthetic": []}
    sizes = (1, 1000, 100_000)

    n = a.explicit_rows
    rows = rng.standard_normal((min(n, 1 << 20), D), dtype=np.float32)
    all_ids = rng.permutation(4 * n).astype(np.int64)[:n]
    pick = lambda c, g: g.choice(all_ids, c, replace=False)  # noqa: E731
    for screen, mid in COPIES:
        s = explicit_searcher(ctx, rows, all_ids, screen, mid)
        out["explicit"].append({"rows": n, "screen": screen, "mid": mid, "runs": [latency(s, pick, c, rng) for c in sizes]})
        if mid == "off":
            q = rng.standard_normal((64, D), dtype=np.float32)
            before = step(s, q, a.steps)
            ids = pick(n // 100, rng)
            vecs = rng.standard_normal((ids.size, D), dtype=np.float32)
            t0 = time.perf_counter()
            s.update_items(ids, vecs)
            upd_ms = (time.perf_counter() - t0) * 1e3
            after = step(s, q, a.steps)
            out["step"] = {"rows": n, "B": 64, "k": 10, "updated": int(ids.size), "update_ms": upd_ms, "before": before, "after": after}
            # the same source rebuilt: staged under PCV_STAGING_SOURCE, swapped in, finalized (Searcher.rebuild_source's calls)
            lib = _ffi.lib()
            t0 = time.perf_counter()
            fill(s, pa.search.STAGING_SOURCE, rows, all_ids)
            _ffi.check(lib.pcv_searcher_replace_source(s._handle, C.c_int64(pa.search.STAGING_SOURCE), C.c_int64(1)))
            s.finalize()
            out["rebuild"] = {"rows": n, "screen": screen, "mid": mid, "ms": (time.perf_counter() - t0) * 1e3}
        s.close()
    del rows

    n = a.synthetic_rows
    for screen, mid in COPIES:
        s = pa.Searcher(ctx, D, "cosine")
        s.set_screening_copy(screen)
        s.set_mid_copy(mid)
        s.add_synthetic(1, n, 0x5EED)
        s.finalize()
        out["synthetic"].append({"rows": n, "screen": screen, "mid": mid,
                                 "runs": [latency(s, lambda c, g: g.choice(n, c, replace=False), c, rng) for c in sizes]})
        s.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
