#!/usr/bin/env python3
"""The linkage tree (pcv_searcher_linkage_tree) beside neighbors(k = 1), whose bound pass, list pass and rescore do for every row what
round 0 of the tree does for every component of one row: the yardstick of a round.

    python tools/bench_linkage.py [--rows 100000] [--corpus clustered|gaussian] [--topics 200] [--topic-rows 2000]
                                  [--repeats 3] [--warmup 1]

A cosine searcher of --rows x 384 rows.  clustered: the corpus of tools/bench_density.py, --topics centres with --topic-rows rows each
at cosine about 0.9 of their centre (scaled down with --rows when they do not fit), shuffled among Gaussian filler; gaussian: plain
Gaussian rows.  Two legs on the same searcher, in the same process, alternating (measuring-on-mi355x: warm-up, several repeats,
alternating order):
  A  linkage_tree(None);
  B  neighbors(None, 1).
Every time is a hipEvent time of the library's stats, or a host clock around a call that ends in a device synchronise.  The rounds
come from PCV_LINKAGE_ROUNDS_FILE, which makes the library append one line per round.
Prints one JSON line: wall seconds of both legs (median, min, max), the per-step ms of the tree summed over the rounds, the rounds
and per round the components, candidates and ms, round 0's bound + list + rescore over leg B's bound + screen + rescore (ratio and
spread), the whole call over (rounds) x leg B, and the last pcv_linkage_stats.  Nothing is asserted.  Progress goes to stderr."""
import argparse
import json
import os
import sys
import tempfile
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
    centres = rng.standard_normal((max(topics, 1), D))
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
        rows[member] = (0.9 * centres[t[member]] + np.sqrt(0.19 / D) * rows[member]).astype(np.float32)
        s.add_rows(1, rows, np.arange(r0, r0 + m, dtype=np.int64))
        print("built %d rows" % (r0 + m), file=sys.stderr, flush=True)
    s.finalize()
    return s


def read_rounds(path):
    out = []
    for line in open(path):
        f = line.split()
        out.append({"round": int(f[0]), "components": int(f[1]), "components_after": int(f[2]), "candidates": int(f[3]),
                    "bound_repeated": int(f[4]), "list_repeated": int(f[5]), "bound_ms": float(f[6]), "list_ms": float(f[7]),
                    "rescore_ms": float(f[8]), "merge_ms": float(f[9])})
    open(path, "w").close()
    return out


def leg_tree(s, log):
    t0 = time.perf_counter()
    tree = s.linkage_tree(None)
    dt = time.perf_counter() - t0
    return dt, s.last_linkage_stats(), read_rounds(log), len(tree[6])


def leg_neighbors(s):
    t0 = time.perf_counter()
    s.neighbors(None, 1)
    return time.perf_counter() - t0, s.last_neighbor_stats()


def spread(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--corpus", choices=("clustered", "gaussian"), default="clustered")
    ap.add_argument("--topics", type=int, default=200)
    ap.add_argument("--topic-rows", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    topics, topic_rows = (a.topics, a.topic_rows) if a.corpus == "clustered" else (0, 0)
    if topics * topic_rows > a.rows * 2 // 5:  # (the density bench's share of topic rows: 40 per cent)
        topic_rows = max(1, a.rows * 2 // 5 // topics)
    log = tempfile.NamedTemporaryFile(prefix="linkage_rounds_", suffix=".txt", delete=False)
    log.close()
    os.environ["PCV_LINKAGE_ROUNDS_FILE"] = log.name
    ctx = pa.Context(0)
    s = build(ctx, a.rows, topics, topic_rows, 11)
    for _ in range(a.warmup):
        leg_tree(s, log.name)
        leg_neighbors(s)
    trees, nbrs = [], []
    for i in range(a.repeats):  # A B, B A, A B, ...
        order = ("tree", "nbr") if i % 2 == 0 else ("nbr", "tree")
        for leg in order:
            if leg == "tree":
                trees.append(leg_tree(s, log.name))
            else:
                nbrs.append(leg_neighbors(s))
        print("repeat %d: linkage_tree %.3f s (%d rounds), neighbors(1) %.3f s" % (i, trees[-1][0], trees[-1][1]["rounds"], nbrs[-1][0]),
              file=sys.stderr, flush=True)
    os.unlink(log.name)
    st = trees[-1][1]
    round0 = np.array([r[2][0]["bound_ms"] + r[2][0]["list_ms"] + r[2][0]["rescore_ms"] for r in trees])
    leg_b = np.array([r[1]["bound_ms"] + r[1]["screen_ms"] + r[1]["rescore_ms"] for r in nbrs])
    tree_ms = np.array([r[1]["bound_ms"] + r[1]["list_ms"] + r[1]["rescore_ms"] + r[1]["merge_ms"] for r in trees])
    out = {
        "metric": "linkage_tree beside neighbors(k = 1) (ms)", "rows": s.num_rows, "dim": D, "corpus": a.corpus, "topics": topics,
        "topic_rows": topic_rows, "edges": trees[-1][3], "rounds": st["rounds"],
        "linkage_tree_s": spread([r[0] for r in trees]), "neighbors_s": spread([r[0] for r in nbrs]),
        "prep_ms": spread([r[1]["prep_ms"] for r in trees]), "bound_ms": spread([r[1]["bound_ms"] for r in trees]),
        "list_ms": spread([r[1]["list_ms"] for r in trees]), "rescore_ms": spread([r[1]["rescore_ms"] for r in trees]),
        "merge_ms": spread([r[1]["merge_ms"] for r in trees]),
        "per_round": trees[-1][2],
        "round0_ms": spread(round0), "neighbors_bound_list_rescore_ms": spread(leg_b),
        "round0_over_neighbors": float(np.median(round0) / np.median(leg_b)),
        "round0_over_neighbors_range": [float(round0.min() / leg_b.max()), float(round0.max() / leg_b.min())],
        "neighbors_spread_rel": float((leg_b.max() - leg_b.min()) / np.median(leg_b)),
        "tree_over_rounds_x_neighbors": float(np.median(tree_ms) / (st["rounds"] * np.median(leg_b))),
        "neighbor_stats": nbrs[-1][1], "stats": st,
    }
    print(json.dumps(out), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
