#!/usr/bin/env python3
"""Compound queries (pcv_searcher_search_compound): what the select step costs beside the scan pass it follows, and how far a walk
goes before its certificate holds.

    python tools/bench_compound.py [--rows 10000000] [--steps 20] [--warmup 3] [--k 10] [--pairs 32]

A cosine searcher of --rows x 384 synthetic rows under AUTO (item id = row number, no id column); the vectors are stored rows plus
noise, or Gaussian.

(1) Per launch, from hipEvents recorded right before and after every select step (pcv_searcher_last_select_stats) and, for the pass
    it follows, from the events of the pass pipeline (pcv_searcher_last_stats: total_ms), in the same call — pool = 128, so one pass
    and one select launch per call; --steps calls after --warmup, median and quartiles:
      a  16 compounds of W = 2, A = 0 in one group (32 part queries);
      b  16 compounds of W = 8, A = 8 in one group (128 part queries);
      b0 the same without the avoided vectors (W = 8, A = 0): the same candidates, row reads and rank counting, 9 instead of 17
         f64 chains a row — b - b0 is what eight chains cost, and what is left of b0 is the row reads and the counting;
      c  search_boosted with a zero boost over the 32 vectors of (a): boost_select_kernel, one workgroup per query.
(2) Entries walked per list until the certificate holds, k results, pool 4096, both modes: --pairs pairs of Gaussian vectors, and
    --pairs pairs of planted neighbours (a stored row plus noise, and its nearest other row plus noise).  Measured once per run.
Prints one JSON line."""
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
SEG = 2_500_000  # rows per synthetic segment


def spread(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "q1": float(np.percentile(x, 25)), "q3": float(np.percentile(x, 75)),
            "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def per_launch(s, fn, warmup, steps):
    """fn: one ranked call of one pass -> (select ms per launch, pass ms per launch), one sample per call"""
    select, scan = [], []
    for i in range(warmup + steps):
        fn()
        ms, launches = s.last_select_stats()
        stats = s.last_stats()
        assert launches >= 1
        if i >= warmup:
            select.append(ms / launches)
            scan.append(stats["total_ms"] / max(1, stats["scan_launches"]))
    return select, scan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=32)
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    for r0 in range(0, a.rows, SEG):
        s.add_synthetic(1, min(SEG, a.rows - r0), 0x5EED, first_row=r0)
    s.finalize()
    rng = np.random.default_rng(3)
    stored, _ = s.get_rows(rng.integers(0, a.rows, size=256).astype(np.int64))
    noisy = (stored + 0.05 * rng.standard_normal(stored.shape)).astype(np.float32)
    # ---- (1) the select step beside its pass ----
    w2 = [noisy[2 * i : 2 * i + 2] for i in range(16)]
    w8 = [noisy[8 * i : 8 * i + 8] for i in range(16)]
    a8 = [noisy[128 + 8 * i : 136 + 8 * i] for i in range(16)]
    flat = np.concatenate(w2)
    got = s.search_compound(None, a.k, w2, None, "any", 1.0, 128)
    assert (got[4] == a.k).all() and s.last_select_stats()[1] == 1
    sel_a, scan_a = per_launch(s, lambda: s.search_compound(None, a.k, w2, None, "all", 1.0, 128), a.warmup, a.steps)
    sel_b, scan_b = per_launch(s, lambda: s.search_compound(None, a.k, w8, a8, "all", 0.5, 128), a.warmup, a.steps)
    sel_b0, scan_b0 = per_launch(s, lambda: s.search_compound(None, a.k, w8, None, "all", 0.5, 128), a.warmup, a.steps)
    sel_c, scan_c = per_launch(s, lambda: s.search_boosted(None, a.k, flat, [0], [0.0], 0.0, 128), a.warmup, a.steps)
    # ---- (2) entries until the certificate holds ----
    n = a.pairs
    gauss = [rng.standard_normal((2, D)).astype(np.float32) for _ in range(n)]
    near_ids, _sc, _cnt = s.search_vectors(None, 2, stored[:n])
    near, _ = s.get_rows(near_ids[:, 1].astype(np.int64))
    planted = [np.stack([noisy[i], (near[i] + 0.05 * rng.standard_normal(D)).astype(np.float32)]) for i in range(n)]
    need = {}
    for name, pairs in (("gaussian_pairs", gauss), ("planted_neighbour_pairs", planted)):
        for mode in ("all", "any"):
            r = s.search_compound(None, a.k, pairs, None, mode, 1.0, 4096)
            ms, launches = s.last_select_stats()
            need[name + "_" + mode] = {"examined": spread(r[5]), "certified": int(r[6].sum()), "compounds": n,
                                       "select_ms_per_launch": ms / max(1, launches), "launches": launches}
    print(json.dumps({
        "metric": "compound select step vs its scan pass vs boost_select_kernel (hipEvent ms per launch)",
        "rows": s.num_rows, "dim": D, "k": a.k,
        "w2_x16_select_ms": spread(sel_a), "w2_x16_pass_ms": spread(scan_a),
        "w8_a8_x16_select_ms": spread(sel_b), "w8_a8_x16_pass_ms": spread(scan_b),
        "w8_a0_x16_select_ms": spread(sel_b0), "w8_a0_x16_pass_ms": spread(scan_b0),
        "boost_x32_select_ms": spread(sel_c), "boost_x32_pass_ms": spread(scan_c),
        "select_over_pass": {"w2_x16": float(np.median(sel_a) / np.median(scan_a)), "w8_a8_x16": float(np.median(sel_b) / np.median(scan_b))},
        "screen_bits": s.last_stats()["screen_bits"], "entries_until_certified": need, "date": time.strftime("%Y-%m-%d"),
    }), flush=True)
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
