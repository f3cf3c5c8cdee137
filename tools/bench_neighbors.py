#!/usr/bin/env python3
"""Item neighbours (pcv_searcher_neighbors) beside the only way to get the same table without it: batches of 256 ids through
search_like with the examples excluded.

    python tools/bench_neighbors.py [--rows 1000000] [--k 10] [--repeats 2] [--baseline-repeats 2] [--warmup 0]

A cosine searcher of --rows x 384 synthetic rows with the copies AUTO builds (int8 screening copy, the mid copy waited for).  Two
legs on the same searcher, in the same process, in the order A B B A (measuring-on-mi355x: alternating order, spread reported):
  A  neighbors(k): one call;
  B  for every 256 consecutive ids: search_like(k, exclude_examples=True) — N / 256 passes over the screening copy, each with its
     fixed cost and its host round trip.
The neighbour ids of the two legs are compared for equality (both are exact under the canonical cosine; a difference is reported,
not hidden).  Prints one JSON line: wall seconds of both legs (median, min, max, by order), the step times of A from
pcv_neighbor_stats, candidates per row, and the bytes per second of A's two screen launches.  Progress goes to stderr."""
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
BATCH = 256


def leg_a(s, k):
    t0 = time.perf_counter()
    ids, nbr, _scores, counts = s.neighbors(None, k)
    dt = time.perf_counter() - t0
    st = s.last_neighbor_stats()
    print("A %.3f s %s" % (dt, st), file=sys.stderr, flush=True)
    return dt, ids, nbr, counts, st


def leg_b(s, k, ids):
    t0 = time.perf_counter()
    out = np.full((len(ids), k), -1, dtype=np.int64)
    for i0 in range(0, len(ids), BATCH):
        chunk = ids[i0 : i0 + BATCH]
        got, _scores, counts, found = s.search_like(None, k, chunk.reshape(-1, 1).tolist(), exclude_examples=True)
        assert found.all()
        out[i0 : i0 + len(chunk)] = got
    dt = time.perf_counter() - t0
    print("B %.3f s" % dt, file=sys.stderr, flush=True)
    return dt, out


def spread(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--baseline-repeats", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=0)
    ap.add_argument("--skip-baseline", action="store_true")
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, a.rows, 0x4E42)
    s.finalize()
    s.wait_background()
    for _ in range(a.warmup):
        leg_a(s, a.k)
    half = max(1, a.repeats // 2)
    a1 = [leg_a(s, a.k) for _ in range(half)]
    b_runs = []
    if not a.skip_baseline:
        b_runs = [leg_b(s, a.k, a1[0][1]) for _ in range(a.baseline_repeats)]
    a2 = [leg_a(s, a.k) for _ in range(a.repeats - half)]
    runs = a1 + a2
    _dt, ids, nbr, counts, st = runs[-1]
    blocks = (a.rows + 31) // 32
    tiles = (blocks + st["tile_rows"] // 32 - 1) // (st["tile_rows"] // 32)
    block_bytes = 32 * D * 4
    bound_bytes = tiles * ((blocks + st["sample_stride"] - 1) // st["sample_stride"]) * block_bytes
    list_bytes = tiles * blocks * block_bytes * (1 + st["reruns"])
    out = {
        "metric": "neighbors vs search_like in batches of %d (wall s)" % BATCH, "rows": s.num_rows, "dim": D, "k": a.k,
        "neighbors_s": spread([r[0] for r in runs]),
        "neighbors_by_order_s": [float(np.median([r[0] for r in a1])), float(np.median([r[0] for r in a2]))] if a2 else None,
        "stats": st, "candidates_per_row": st["candidates"] / max(1, st["rows"]),
        "bound_bytes_per_s": bound_bytes / (st["bound_ms"] * 1e-3) if st["bound_ms"] > 0 else None,
        "list_bytes_per_s": list_bytes / (st["screen_ms"] * 1e-3) if st["screen_ms"] > 0 else None,
        "all_counts_k": bool((counts == a.k).all()),
    }
    if b_runs:
        nbr_b = b_runs[-1][1]
        out["baseline_s"] = spread([r[0] for r in b_runs])
        out["neighbor_ids_equal"] = bool(np.array_equal(nbr, nbr_b))
        out["rows_that_differ"] = int((nbr != nbr_b).any(axis=1).sum())
        out["speedup_median"] = out["baseline_s"]["median"] / out["neighbors_s"]["median"]
    print(json.dumps(out), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
