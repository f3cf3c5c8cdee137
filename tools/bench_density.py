#!/usr/bin/env python3
"""Density clusters (pcv_searcher_density_clusters) beside the duplicate-pair screen, whose kernel streams the same bytes through
the same MFMA loop and is the yardstick of the two screen passes of a density call.

    python tools/bench_density.py [--rows 1000000] [--topics 200] [--topic-rows 2000] [--threshold 0.75] [--min-items 10]
                                  [--duplicate-threshold 0.95] [--repeats 5] [--warmup 1]

A cosine searcher of --rows x 384 rows: --topics centres with --topic-rows rows each at cosine about 0.9 of their centre (about 0.81
of each other: far above the threshold, so the screen decides nearly every near pair alone), shuffled among Gaussian filler.  Two
legs on the same searcher, in the same process, alternating (measuring-on-mi355x: warm-up, several repeats, alternating order):
  A  density_clusters(threshold, min_items);
  B  find_duplicates(duplicate_threshold): a threshold no pair reaches, so that it stays under its pair cap — its screen_ms is the
     cost of streaming the upper triangle once.
Prints one JSON line: wall seconds of both legs, degree_ms, link_ms and screen_ms (median, min, max), the two ratios degree_ms /
screen_ms and link_ms / screen_ms, the share of near pairs decided without f64, sure_pairs / (sure_pairs + confirmed), and the last
pcv_density_stats.  Progress goes to stderr."""
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


def build(ctx, n, topics, topic_rows, seed):
    rng = np.random.default_rng(seed)
    assert topics * topic_rows <= n
    centres = rng.standard_normal((topics, D))
    centres /= np.linalg.norm(centres, axis=1)[:, None]
    topic_of = np.full(n, -1, dtype=np.int64)
    topic_of[rng.permutation(n)[: topics * topic_rows]] = np.repeat(np.arange(topics), topic_rows)
    s = pa.Searcher(ctx, D, "cosine")
    s.reserve(1, n)
    for r0 in range(0, n, CHUNK):
        m = min(CHUNK, n - r0)
        rows = rng.standard_normal((m, D)).astype(np.float32)
        t = topic_of[r0 : r0 + m]
        member = t >= 0
        # 0.9 c + sqrt(0.19) g / |g|-ish: |g| is sqrt(D) within a few per cent
        rows[member] = (0.9 * centres[t[member]] + np.sqrt(0.19 / D) * rows[member]).astype(np.float32)
        s.add_rows(1, rows, np.arange(r0, r0 + m, dtype=np.int64))
        print("built %d rows" % (r0 + m), file=sys.stderr, flush=True)
    s.finalize()
    return s, topic_of


def leg_density(s, threshold, min_items):
    t0 = time.perf_counter()
    _ids, labels, kinds, _degrees, clusters = s.density_clusters(None, threshold, min_items)
    return time.perf_counter() - t0, s.last_density_stats(), labels, kinds, clusters


def leg_duplicates(s, threshold):
    t0 = time.perf_counter()
    _a, _b, _scores, total = s.find_duplicates(None, threshold, max_pairs=1 << 20)
    return time.perf_counter() - t0, s.last_duplicate_stats(), total


def spread(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--topics", type=int, default=200)
    ap.add_argument("--topic-rows", type=int, default=2000)
    ap.add_argument("--threshold", type=float, default=0.75)
    ap.add_argument("--min-items", type=int, default=10)
    ap.add_argument("--duplicate-threshold", type=float, default=0.95)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    ctx = pa.Context(0)
    s, topic_of = build(ctx, a.rows, a.topics, a.topic_rows, 11)
    for _ in range(a.warmup):
        leg_density(s, a.threshold, a.min_items)
        leg_duplicates(s, a.duplicate_threshold)
    dens, dups = [], []
    for i in range(a.repeats):  # A B, B A, A B, ...
        order = (leg_density, leg_duplicates) if i % 2 == 0 else (leg_duplicates, leg_density)
        for leg in order:
            if leg is leg_density:
                dens.append(leg_density(s, a.threshold, a.min_items))
            else:
                dups.append(leg_duplicates(s, a.duplicate_threshold))
        print("repeat %d: density %.3f s, duplicates %.3f s" % (i, dens[-1][0], dups[-1][0]), file=sys.stderr, flush=True)
    st = dens[-1][1]
    labels, kinds, clusters = dens[-1][2:]
    # every topic one cluster of its own, the filler noise (reported, not assumed)
    member = topic_of >= 0
    per_topic = [np.unique(labels[topic_of == t]) for t in range(a.topics)]
    degree_ms = np.array([r[1]["degree_ms"] for r in dens])
    link_ms = np.array([r[1]["link_ms"] for r in dens])
    screen_ms = np.array([r[1]["screen_ms"] for r in dups])
    blocks = (a.rows + 31) // 32
    tile_blocks = st["tile_rows"] // 32
    streamed = sum(blocks - t for t in range(0, blocks, tile_blocks)) * 32 * D * 4  # blocks at and after each tile's first block
    near = st["sure_pairs"] + st["confirmed"]
    out = {
        "metric": "density_clusters beside find_duplicates' screen (ms)", "rows": s.num_rows, "dim": D, "threshold": a.threshold,
        "min_items": a.min_items, "topics": a.topics, "topic_rows": a.topic_rows, "clusters": int(clusters),
        "topics_in_one_cluster_each": bool(all(len(u) == 1 and u[0] >= 0 for u in per_topic)
                                           and len({int(u[0]) for u in per_topic if len(u) == 1}) == a.topics),
        "filler_rows_noise": int((kinds[~member] == pa.PCV_DENSITY_NOISE).sum()), "filler_rows": int((~member).sum()),
        "density_s": spread([r[0] for r in dens]), "find_duplicates_s": spread([r[0] for r in dups]),
        "degree_ms": spread(degree_ms), "link_ms": spread(link_ms), "rescore_ms": spread([r[1]["rescore_ms"] for r in dens]),
        "label_ms": spread([r[1]["label_ms"] for r in dens]), "screen_ms": spread(screen_ms),
        "degree_over_screen": float(np.median(degree_ms) / np.median(screen_ms)),
        "link_over_screen": float(np.median(link_ms) / np.median(screen_ms)),
        "screen_spread_rel": float((screen_ms.max() - screen_ms.min()) / np.median(screen_ms)),
        "decided_without_f64": near and st["sure_pairs"] / near,
        "duplicate_pairs": int(dups[-1][2]), "duplicate_candidates": int(dups[-1][1]["candidates"]),
        "stats": st, "screen_bytes": streamed,
        "screen_bytes_per_s": streamed / (float(np.median(screen_ms)) * 1e-3),
    }
    print(json.dumps(out), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
