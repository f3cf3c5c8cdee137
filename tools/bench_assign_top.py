#!/usr/bin/env python3
"""Top-m labels (pcv_searcher_assign_top) beside plain assign on the same corpus.

    python tools/bench_assign_top.py [--rows 1000000] [--labels 128] [--repeats 5] [--warmup 1]

A cosine searcher of --rows x 384 synthetic rows with the screening copy off and --labels labels taken from stored items (get_rows).
In one process, alternating (warm-up, several repeats, both orders): plain assign, then assign_top for m in {1, 2, 4, 8} without a
bound and with min_score = 0.3.  Prints one JSON line: the step times of assign (prep / screen / rescore) and of every assign_top
form (prep / bound / screen / rescore / select; median, min, max), candidates per row, the labels listed per row, and the bytes/s of
the new screen — its bound and list passes stream N x D x 4 bytes each per label tile — as a fraction of 8 TB/s.  The two-pass
screen is expected near twice assign's screen plus the select step; it is reported, not gated."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import perceive_amd as pa  # noqa: E402

D = 384
PEAK = 8e12  # bytes per second
STEPS = ("prep_ms", "bound_ms", "screen_ms", "rescore_ms", "select_ms")


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--labels", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    ctx = pa.Context(0)
    s = pa.Searcher(ctx, D, "cosine")
    s.set_screening_copy("off")
    s.add_synthetic(1, a.rows, 0xA551)
    s.finalize()
    rng = np.random.default_rng(1)
    pick = np.sort(rng.choice(a.rows, size=a.labels, replace=False)).astype(np.int64)
    labels = np.ascontiguousarray(s.get_rows(pick)[0])
    nbytes = a.rows * D * 4
    forms = [(m, bound) for bound in (None, 0.3) for m in (1, 2, 4, 8)]

    def plain():
        s.assign(None, labels)
        return s.last_assign_stats()

    def top(form):
        s.assign_top(None, labels, form[0], form[1])
        return s.last_assign_top_stats()

    for _ in range(a.warmup):
        plain()
        for f in forms:
            top(f)
    base, runs = [], {f: [] for f in forms}
    for r in range(a.repeats):
        order = forms if r % 2 == 0 else forms[::-1]
        if r % 2 == 0:
            base.append(plain())
        for f in order:
            runs[f].append(top(f))
        if r % 2 == 1:
            base.append(plain())
    screen = float(np.median([x["screen_ms"] for x in base]))
    out = {
        "metric": "assign_top (m best of K labels) vs assign (ms)", "rows": a.rows, "dim": D, "labels": a.labels,
        "assign": {k: spread([x[k] for x in base]) for k in ("prep_ms", "screen_ms", "rescore_ms")},
        "assign_candidates_per_row": base[-1]["candidates"] / a.rows,
        "assign_screen_fraction_of_8TBs": nbytes * base[-1]["label_tiles"] / (screen * 1e-3) / PEAK,
        "forms": [],
    }
    for f in forms:
        st = runs[f]
        two = float(np.median([x["bound_ms"] + x["screen_ms"] for x in st]))
        total = float(np.median([sum(x[k] for k in STEPS) for x in st]))
        row = {"m": f[0], "min_score": f[1], "candidates_per_row": st[-1]["candidates"] / a.rows, "listed_per_row": st[-1]["listed"] / a.rows,
               "reruns": int(st[-1]["reruns"]), "label_tiles": int(st[-1]["label_tiles"]), "steps_ms": total,
               "bound_plus_screen_over_assign_screen": two / screen,
               "screen_fraction_of_8TBs": 2 * nbytes * st[-1]["label_tiles"] / (two * 1e-3) / PEAK}
        row.update({k: spread([x[k] for x in st]) for k in STEPS})
        out["forms"].append(row)
    print(json.dumps(out))
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
