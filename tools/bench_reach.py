#!/usr/bin/env python3
"""The reach tree (pcv_searcher_reach_tree) beside the two existing calls that together do comparable work: neighbors(k = min_items
- 1), whose bound, list and rescore steps the core step runs, followed by linkage_tree, whose rounds the reach rounds are with the
cap applied.

    python tools/bench_reach.py [--rows 100000] [--corpus clustered|gaussian] [--topics 200] [--topic-rows 2000] [--min-items 16]
                                [--repeats 3] [--warmup 1]

A cosine searcher of --rows x 384 rows: the corpora of tools/bench_linkage.py.  Two legs on the same searcher, in the same process,
alternating (measuring-on-mi355x: warm-up, several repeats, alternating order):
  A  reach_tree(None, min_items);
  B  neighbors(None, min_items - 1), then linkage_tree(None).
Every time is a hipEvent time of the library's stats, or a host clock around a call that ends in a device synchronise.  The rounds
come from PCV_LINKAGE_ROUNDS_FILE, which makes the library append one line per round (of either tree).
Prints one JSON line: wall seconds of both legs (median, min, max) and their ratio with its range, the per-step ms of leg A from
pcv_reach_stats, the same steps of leg B from pcv_neighbor_stats and pcv_linkage_stats, per round of either tree the components,
candidates and ms, and the last stats.  A leg that ends in PCV_ERR_UNSUPPORTED (more candidates than a list may hold) is reported
with its message in place of its times.  Nothing is asserted.  Progress goes to stderr."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perceive_amd as pa  # noqa: E402
from bench_linkage import build, read_rounds, spread  # noqa: E402

D = 384


def leg_reach(s, log, min_items):
    t0 = time.perf_counter()
    try:
        tree = s.reach_tree(None, min_items)
    except pa.PcvError as e:
        read_rounds(log)
        return None, str(e), [], 0
    dt = time.perf_counter() - t0
    return dt, s.last_reach_stats(), read_rounds(log), len(tree[7])


def leg_both(s, log, k):
    t0 = time.perf_counter()
    try:
        s.neighbors(None, k)
        t1 = time.perf_counter()
        nst = s.last_neighbor_stats()
        s.linkage_tree(None)
    except pa.PcvError as e:
        read_rounds(log)
        return None, str(e), None, None, []
    t2 = time.perf_counter()
    return t2 - t0, t1 - t0, nst, s.last_linkage_stats(), read_rounds(log)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--corpus", choices=("clustered", "gaussian"), default="clustered")
    ap.add_argument("--topics", type=int, default=200)
    ap.add_argument("--topic-rows", type=int, default=2000)
    ap.add_argument("--min-items", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    assert 2 <= a.min_items <= 65
    topics, topic_rows = (a.topics, a.topic_rows) if a.corpus == "clustered" else (0, 0)
    if topics * topic_rows > a.rows * 2 // 5:  # (the density bench's share of topic rows: 40 per cent)
        topic_rows = max(1, a.rows * 2 // 5 // topics)
    log = tempfile.NamedTemporaryFile(prefix="reach_rounds_", suffix=".txt", delete=False)
    log.close()
    os.environ["PCV_LINKAGE_ROUNDS_FILE"] = log.name
    ctx = pa.Context(0)
    s = build(ctx, a.rows, topics, topic_rows, 11)
    k = a.min_items - 1
    for _ in range(a.warmup):
        leg_reach(s, log.name, a.min_items)
        leg_both(s, log.name, k)
    reach, both = [], []
    for i in range(a.repeats):  # A B, B A, A B, ...
        for leg in ("reach", "both") if i % 2 == 0 else ("both", "reach"):
            if leg == "reach":
                reach.append(leg_reach(s, log.name, a.min_items))
            else:
                both.append(leg_both(s, log.name, k))
        print("repeat %d: reach_tree %s s, neighbors(%d) + linkage_tree %s s" % (i, reach[-1][0], k, both[-1][0]), file=sys.stderr, flush=True)
    os.unlink(log.name)
    out = {"metric": "reach_tree beside neighbors(k = min_items - 1) + linkage_tree", "rows": s.num_rows, "dim": D, "corpus": a.corpus,
           "topics": topics, "topic_rows": topic_rows, "min_items": a.min_items}
    ok_a, ok_b = [r for r in reach if r[0] is not None], [r for r in both if r[0] is not None]
    if ok_a:
        st = ok_a[-1][1]
        out.update({"reach_tree_s": spread([r[0] for r in ok_a]), "edges": ok_a[-1][3], "rounds": st["rounds"],
                    "reach_ms": {f: spread([r[1][f] for r in ok_a]) for f in ("core_ms", "prep_ms", "bound_ms", "list_ms", "rescore_ms", "merge_ms")},
                    "reach_per_round": ok_a[-1][2], "reach_stats": st})
    else:
        out["reach_tree_error"] = reach[-1][1]
    if ok_b:
        nst, lst = ok_b[-1][2], ok_b[-1][3]
        out.update({"neighbors_plus_linkage_s": spread([r[0] for r in ok_b]), "neighbors_s": spread([r[1] for r in ok_b]),
                    "neighbors_ms": {f: spread([r[2][f] for r in ok_b]) for f in ("prep_ms", "bound_ms", "screen_ms", "rescore_ms", "select_ms")},
                    "linkage_ms": {f: spread([r[3][f] for r in ok_b]) for f in ("prep_ms", "bound_ms", "list_ms", "rescore_ms", "merge_ms")},
                    "linkage_per_round": ok_b[-1][4], "neighbor_stats": nst, "linkage_stats": lst})
    else:
        out["neighbors_plus_linkage_error"] = both[-1][1]
    if ok_a and ok_b:
        ta, tb = np.array([r[0] for r in ok_a]), np.array([r[0] for r in ok_b])
        out["reach_over_neighbors_plus_linkage"] = float(np.median(ta) / np.median(tb))
        out["reach_over_neighbors_plus_linkage_range"] = [float(ta.min() / tb.max()), float(ta.max() / tb.min())]
    print(json.dumps(out), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
