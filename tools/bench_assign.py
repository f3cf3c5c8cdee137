#!/usr/bin/env python3
"""Item labels (pcv_searcher_assign, pcv_searcher_kmeans) beside the search pass that reads the same bytes through the same tile.

    python tools/bench_assign.py [--rows 1000000] [--labels 128] [--kmeans-k 256] [--kmeans-iters 10] [--repeats 5] [--warmup 1]

A cosine searcher of --rows x 384 synthetic rows with the screening copy off, so that a 128-query search pass streams the f32 rows
with scan_mfma_kernel — N x D x 4 bytes through a 128-row bf16 tile, what the screen of assign streams for 128 labels.  In one
process, alternating (measuring-on-mi355x: warm-up, several repeats, both orders):
  A  assign with --labels labels taken from stored items (get_rows): prep / screen / rescore times from pcv_assign_stats;
  B  search_vectors of the same 128 vectors, 10 results: scan_ms from pcv_scan_stats.
Then --kmeans-iters k-means updates at K = --kmeans-k from stored items, wall time.  Prints one JSON line: the three step times of A
(median, min, max), the screen's N x D x 4 / time as a fraction of 8 TB/s, B's scan time likewise, and the k-means time per
iteration.  The expectation is that A's screen is not slower than B's scan beyond B's run-to-run spread; it is reported, not gated."""
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
PEAK = 8e12  # bytes per second


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--labels", type=int, default=128)
    ap.add_argument("--kmeans-k", type=int, default=256)
    ap.add_argument("--kmeans-iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    s.set_screening_copy("off")
    s.add_synthetic(1, a.rows, 0xA551)
    s.finalize()
    rng = np.random.default_rng(1)
    pick = np.sort(rng.choice(a.rows, size=max(a.labels, a.kmeans_k, 128), replace=False)).astype(np.int64)
    vecs = s.get_rows(pick)[0]
    labels, queries = np.ascontiguousarray(vecs[: a.labels]), np.ascontiguousarray(vecs[:128])
    nbytes = a.rows * D * 4

    def leg_a():
        s.assign(None, labels)
        return s.last_assign_stats()

    def leg_b():
        s.search_vectors(None, 10, queries)
        return s.last_stats()

    for _ in range(a.warmup):
        leg_a(), leg_b()
    sa, sb = [], []
    for r in range(a.repeats):
        for leg in (("a", "b") if r % 2 == 0 else ("b", "a")):
            (sa if leg == "a" else sb).append(leg_a() if leg == "a" else leg_b())
    screen = [x["screen_ms"] for x in sa]
    scan = [x["scan_ms"] for x in sb]
    out = {
        "metric": "assign (K labels) vs one 128-query f32 search pass (ms)", "rows": a.rows, "dim": D, "labels": a.labels,
        "prep_ms": spread([x["prep_ms"] for x in sa]), "screen_ms": spread(screen), "rescore_ms": spread([x["rescore_ms"] for x in sa]),
        "candidates": int(sa[-1]["candidates"]), "label_tiles": int(sa[-1]["label_tiles"]), "reruns": int(sa[-1]["reruns"]),
        "screen_fraction_of_8TBs": nbytes * sa[-1]["label_tiles"] / (np.median(screen) * 1e-3) / PEAK,
        "search_scan_ms": spread(scan), "search_kernel": int(sb[-1]["kernel_used"]),
        "search_fraction_of_8TBs": nbytes / (np.median(scan) * 1e-3) / PEAK,
        "screen_over_scan": float(np.median(screen) / np.median(scan)),
    }
    if a.kmeans_iters > 0:
        init = np.ascontiguousarray(vecs[: a.kmeans_k])
        t0 = time.perf_counter()
        res = s.kmeans(None, a.kmeans_k, init, max_iters=a.kmeans_iters)
        dt = time.perf_counter() - t0
        out["kmeans"] = {"k": a.kmeans_k, "iterations": int(res[5]), "wall_s": dt, "s_per_iteration": dt / max(1, res[5] + 1),
                         "moved": [int(m) for m in res[6]], "stats": s.last_assign_stats()}
    print(json.dumps(out))
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
