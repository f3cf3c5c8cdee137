#!/usr/bin/env python3
"""Group-aware neighbours (pcv_searcher_neighbors_grouped) beside the only way to get the same table without them: the plain
neighbours with room for the siblings, filtered on the host.

    python tools/bench_pair_groups.py [--rows 1000000] [--k 10] [--chunks 8] [--noise 0.5]

A cosine searcher of --rows x 384 rows: documents of --chunks chunks, each a document vector plus noise (sibling cosines around 0.8 at
the default noise), the group of row i being i // chunks.  Legs on the same searcher, in the same process, in the order A B B A
(measuring-on-mi355x: alternating order, spread reported):
  A  neighbors_grouped(k, SKIP_OWN): one call;
  B  neighbors(k + chunks - 1), then on the host: drop the partners of the owner's group, keep the first k.
The neighbour ids of the two legs are asserted equal.  Beside them, once each: the plain neighbors(k) — its bound pass is the yardstick
for what the tag loads, the compares and the smaller tile cost the grouped one — and neighbors_grouped(k, SKIP_OWN | ONE_PER_GROUP).
Prints one JSON line: wall seconds of both legs (both runs), the step times of every leg from pcv_neighbor_stats, candidates per row
and the counters of pcv_pair_group_stats.  Progress goes to stderr."""
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
STEPS = ("prep_ms", "bound_ms", "screen_ms", "rescore_ms", "select_ms")


def steps(st):
    out = {f: round(float(st[f]), 3) for f in STEPS}
    out.update(candidates=int(st["candidates"]), candidates_per_row=st["candidates"] / max(1, st["rows"]), reruns=int(st["reruns"]),
               stride=int(st["sample_stride"]), spans=int(st["spans"]), tile_rows=int(st["tile_rows"]))
    return out


def leg_grouped(s, k, flags, name):
    t0 = time.perf_counter()
    ids, nbr, _scores, _groups, counts = s.neighbors_grouped(None, k, flags)
    dt = time.perf_counter() - t0
    st, gst = s.last_neighbor_stats(), s.last_pair_group_stats()
    print("%s %.3f s %s %s" % (name, dt, st, gst), file=sys.stderr, flush=True)
    return dt, nbr, counts, steps(st), {f: (round(v, 3) if isinstance(v, float) else int(v)) for f, v in gst.items()}


def leg_filtered(s, k, chunks):
    t0 = time.perf_counter()
    ids, nbr, _scores, _counts = s.neighbors(None, k + chunks - 1)
    t1 = time.perf_counter()
    foreign = (nbr // chunks) != (ids // chunks)[:, None]  # (ids are positions here: the group of id i is i // chunks)
    order = np.argsort(~foreign, axis=1, kind="stable")[:, :k]  # the first k foreign partners, in list order
    out = np.take_along_axis(nbr, order, axis=1)
    dt = time.perf_counter() - t0
    st = s.last_neighbor_stats()
    print("B %.3f s (host filter %.3f s) %s" % (dt, dt - (t1 - t0), st), file=sys.stderr, flush=True)
    return dt, out, dt - (t1 - t0), steps(st), int((~foreign).sum()), bool(foreign[:, : k + chunks - 1].sum(axis=1).min() >= k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--noise", type=float, default=0.5)
    a = ap.parse_args()
    rng = np.random.default_rng(0x9A12)
    n = a.rows
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    ids = np.arange(n, dtype=np.int64)
    docs = rng.standard_normal(((n + a.chunks - 1) // a.chunks, D), dtype=np.float32)
    for lo in range(0, n, 1 << 18):  # a document vector plus noise, 256K rows at a time
        hi = min(n, lo + (1 << 18))
        rows = docs[np.arange(lo, hi) // a.chunks] + np.float32(a.noise) * rng.standard_normal((hi - lo, D), dtype=np.float32)
        s.add_rows(1, rows, ids[lo:hi])
    s.finalize()
    s.wait_background()
    s.set_groups(ids, ids // a.chunks)
    print("built: %d rows, group table %s" % (s.num_rows, s.group_stats()), file=sys.stderr, flush=True)
    SKIP, ONE = pa.GROUPS_SKIP_OWN, pa.GROUPS_ONE_PER_GROUP
    a1 = leg_grouped(s, a.k, SKIP, "A")
    b1 = leg_filtered(s, a.k, a.chunks)
    b2 = leg_filtered(s, a.k, a.chunks)
    a2 = leg_grouped(s, a.k, SKIP, "A")
    assert b1[5] and b2[5], "a row of leg B has fewer than k foreign partners among its k + chunks - 1"
    equal = bool(np.array_equal(a1[1], b1[1]) and np.array_equal(a2[1], b2[1]))
    assert equal, "neighbor ids differ in %d rows" % int((a2[1] != b2[1]).any(axis=1).sum())
    t0 = time.perf_counter()
    s.neighbors(None, a.k)
    plain_s = time.perf_counter() - t0
    plain = steps(s.last_neighbor_stats())
    print("plain k=%d %.3f s %s" % (a.k, plain_s, plain), file=sys.stderr, flush=True)
    both = leg_grouped(s, a.k, SKIP | ONE, "A(3)")
    out = {
        "metric": "neighbors_grouped(k, SKIP_OWN) vs neighbors(k + chunks - 1) filtered on the host (wall s)", "rows": s.num_rows, "dim": D,
        "k": a.k, "chunks": a.chunks, "noise": a.noise,
        "grouped_s": [a1[0], a2[0]], "filtered_s": [b1[0], b2[0]], "host_filter_s": [b1[2], b2[2]],
        "speedup_median": float(np.median([b1[0], b2[0]]) / np.median([a1[0], a2[0]])),
        "neighbor_ids_equal": equal, "all_counts_k": bool((a2[2] == a.k).all()),
        "grouped_steps": [a1[3], a2[3]], "filtered_steps": [b1[3], b2[3]], "group_stats": [a1[4], a2[4]],
        "siblings_in_filtered_lists": b2[4],
        "plain_k_s": plain_s, "plain_k_steps": plain,
        "one_per_group_s": both[0], "one_per_group_steps": both[3], "one_per_group_stats": both[4],
    }
    print(json.dumps(out), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
