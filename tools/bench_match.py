#!/usr/bin/env python3
"""Item matches (pcv_searcher_match) beside the two ways to join two sources without it.

    python tools/bench_match.py [--from-rows 10000] [--to-rows 1000000] [--k 10] [--repeats 2]

A cosine searcher of two sources of 384-d synthetic rows, A (--from-rows) stored before B (--to-rows), with the copies AUTO builds
(int8 screening copy, the mid copy waited for).  Three legs on the same searcher, in the same process, in the order A B C C B A
repeated --repeats / 2 times (measuring-on-mi355x: alternating order, spread reported):
  A  match([A], [B], k): one call;
  B  neighbors(None, k) over the union: it also pays for A x A and B x B, and a row's own source fills its k slots — the table is
     not the same one, only the nearest thing the library had;
  C  for every 256 consecutive ids of A: search_like([B], k) — |A| / 256 passes over B's screening copy, queries built on the device
     (cheaper than reading A's rows back and sending them through search_vectors).
The match ids of A and C are compared for equality (both are exact under the canonical cosine; a difference is reported, not
hidden).  Prints one JSON line: wall seconds of the legs (median, min, max), the step times of A from pcv_match_stats and of B from
pcv_neighbor_stats.  Progress goes to stderr."""
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


def leg_match(s, k):
    t0 = time.perf_counter()
    ids, mids, _scores, counts = s.match([1], [2], k)
    dt = time.perf_counter() - t0
    st = s.last_match_stats()
    print("match %.3f s %s" % (dt, st), file=sys.stderr, flush=True)
    return dt, ids, mids, counts, st


def leg_union(s, k):
    t0 = time.perf_counter()
    s.neighbors(None, k)
    dt = time.perf_counter() - t0
    st = s.last_neighbor_stats()
    print("neighbors over the union %.3f s %s" % (dt, st), file=sys.stderr, flush=True)
    return dt, st


def leg_search(s, k, ids):
    t0 = time.perf_counter()
    out = np.full((len(ids), k), -1, dtype=np.int64)
    for i0 in range(0, len(ids), BATCH):
        chunk = ids[i0 : i0 + BATCH]
        got, _scores, _counts, found = s.search_like([2], k, chunk.reshape(-1, 1).tolist(), exclude_examples=False)
        assert found.all()
        out[i0 : i0 + len(chunk)] = got
    dt = time.perf_counter() - t0
    print("search_like in batches %.3f s" % dt, file=sys.stderr, flush=True)
    return dt, out


def spread(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--from-rows", type=int, default=10_000)
    ap.add_argument("--to-rows", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--skip-union", action="store_true")
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, a.from_rows, 0x4D41)
    s.add_synthetic(2, a.to_rows, 0x4D42, first_row=a.from_rows)
    s.finalize()
    s.wait_background()
    m_runs, u_runs, c_runs = [], [], []
    for _ in range(max(1, a.repeats // 2)):
        m_runs.append(leg_match(s, a.k))
        if not a.skip_union:
            u_runs.append(leg_union(s, a.k))
        c_runs.append(leg_search(s, a.k, m_runs[0][1]))
        c_runs.append(leg_search(s, a.k, m_runs[0][1]))
        if not a.skip_union:
            u_runs.append(leg_union(s, a.k))
        m_runs.append(leg_match(s, a.k))
    _dt, _ids, mids, counts, st = m_runs[-1]
    out = {
        "metric": "match vs neighbors over the union vs search_like in batches of %d (wall s)" % BATCH, "from_rows": a.from_rows,
        "to_rows": a.to_rows, "dim": D, "k": a.k, "match_s": spread([r[0] for r in m_runs]), "match_stats": st,
        "candidates_per_row": st["candidates"] / max(1, st["rows"]), "all_counts_k": bool((counts == a.k).all()),
        "search_s": spread([r[0] for r in c_runs]), "match_ids_equal_search": bool(np.array_equal(mids, c_runs[-1][1])),
        "rows_that_differ": int((mids != c_runs[-1][1]).any(axis=1).sum()),
    }
    out["search_over_match"] = out["search_s"]["median"] / out["match_s"]["median"]
    if u_runs:
        out["union_s"] = spread([r[0] for r in u_runs])
        out["union_stats"] = u_runs[-1][1]
        out["union_over_match"] = out["union_s"]["median"] / out["match_s"]["median"]
    print(json.dumps(out), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
