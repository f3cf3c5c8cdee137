#!/usr/bin/env python3
"""Duplicate pairs (pcv_searcher_find_duplicates) beside the only way to get the same pairs without it: batches of 256 ids through
like_queries + search_range.

    python tools/bench_duplicates.py [--rows 1000000] [--threshold 0.95] [--repeats 5] [--baseline-repeats 2] [--warmup 1]

A cosine searcher of --rows x 384 Gaussian rows of which 1 % are near-copies of other rows (the row plus a tenth of its size in
noise: cosine about 0.995).  Two legs on the same searcher, in the same process, in the order A B B A (measuring-on-mi355x: warm-up,
several repeats, alternating order):
  A  find_duplicates(threshold), max_pairs large enough for every pair;
  B  for every 256 consecutive ids: like_queries, then search_range with the cosine bound and room for 64 hits — each pair comes out
     twice, and the item itself once.
The pair sets of the two legs are compared (B's bound is on the f32 score, A's on the f64 cosine: a pair whose cosine rounds up to
the threshold would be in B alone — the planted pairs are nowhere near it, and a difference is reported, not hidden).  Prints one
JSON line: wall seconds of both legs (median, min, max, by order), the kernel split of A from pcv_duplicate_stats and the bytes
per second of its screen kernel."""
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
CHUNK = 250_000
BATCH = 256


def build(ctx, n, seed):
    rng = np.random.default_rng(seed)
    s = pa.Searcher(ctx, D, "cosine")
    s.reserve(1, n)
    n_copies = n // 100
    dst = np.sort(rng.choice(np.arange(n // 2, n), size=n_copies, replace=False))  # the copies live in the second half,
    src = rng.integers(0, n // 2, size=n_copies)                                  # their originals in the first
    originals = np.empty((n_copies, D), dtype=np.float32)
    for r0 in range(0, n, CHUNK):
        rows = rng.standard_normal((min(CHUNK, n - r0), D)).astype(np.float32)
        here = (src >= r0) & (src < r0 + rows.shape[0])
        originals[here] = rows[src[here] - r0]
        lo, hi = np.searchsorted(dst, r0), np.searchsorted(dst, r0 + rows.shape[0])
        rows[dst[lo:hi] - r0] = originals[lo:hi] + 0.1 * rng.standard_normal((hi - lo, D)).astype(np.float32)
        s.add_rows(1, rows, np.arange(r0, r0 + rows.shape[0], dtype=np.int64))
    s.finalize()
    return s, n_copies


def leg_a(s, threshold, max_pairs):
    t0 = time.perf_counter()
    a, b, _scores, total = s.find_duplicates(None, threshold, max_pairs=max_pairs)
    dt = time.perf_counter() - t0
    assert total == len(a), "max_pairs too small for %d pairs" % total
    return dt, set(zip(a.tolist(), b.tolist())), s.last_duplicate_stats()


def leg_b(s, threshold, n):
    t0 = time.perf_counter()
    pairs = set()
    for i0 in range(0, n, BATCH):
        ids = np.arange(i0, min(n, i0 + BATCH), dtype=np.int64)
        vec, found, _members = s.like_queries([[int(i)] for i in ids])
        assert found.all()
        got, _scores, counts, more = s.search_range(None, threshold, vec, 64)
        assert not more.any()
        for q in np.nonzero(counts > 1)[0]:
            for other in got[q, : counts[q]].tolist():
                if other != ids[q]:
                    pairs.add((min(int(ids[q]), other), max(int(ids[q]), other)))
    return time.perf_counter() - t0, pairs


def spread(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--threshold", type=float, default=0.95)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-repeats", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-baseline", action="store_true")
    a = ap.parse_args()
    ctx = pa.Context(0)
    s, n_copies = build(ctx, a.rows, 7)
    max_pairs = min(1 << 24, max(1024, 8 * n_copies))
    for _ in range(a.warmup):
        leg_a(s, a.threshold, max_pairs)
    half = max(1, a.repeats // 2)
    a1 = [leg_a(s, a.threshold, max_pairs) for _ in range(half)]
    b_runs = []
    if not a.skip_baseline:
        b_runs = [leg_b(s, a.threshold, a.rows) for _ in range(a.baseline_repeats)]
    a2 = [leg_a(s, a.threshold, max_pairs) for _ in range(a.repeats - half)]
    runs = a1 + a2
    pairs_a, st = runs[-1][1], runs[-1][2]
    blocks = (a.rows + 31) // 32
    tile_blocks = st["tile_rows"] // 32
    # blocks a tile streams: those at and after its first block
    streamed = sum(blocks - t for t in range(0, blocks, tile_blocks)) * 32 * D * 4
    out = {
        "metric": "find_duplicates vs like_queries + search_range in batches of %d (wall s)" % BATCH, "rows": s.num_rows, "dim": D,
        "threshold": a.threshold, "planted_copies": n_copies, "pairs": len(pairs_a),
        "find_duplicates_s": spread([r[0] for r in runs]),
        "find_duplicates_by_order_s": [float(np.median([r[0] for r in a1])), float(np.median([r[0] for r in a2]))] if a2 else None,
        "stats": st, "screen_bytes": streamed,
        "screen_bytes_per_s": streamed / (st["screen_ms"] * 1e-3) if st["screen_ms"] > 0 else None,
    }
    if b_runs:
        pairs_b = b_runs[-1][1]
        out["baseline_s"] = spread([r[0] for r in b_runs])
        out["pair_sets_equal"] = pairs_a == pairs_b
        out["only_in_find_duplicates"] = len(pairs_a - pairs_b)
        out["only_in_baseline"] = len(pairs_b - pairs_a)
        out["speedup_median"] = out["baseline_s"]["median"] / out["find_duplicates_s"]["median"]
    print(json.dumps(out), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
