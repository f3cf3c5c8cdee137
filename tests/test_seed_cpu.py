"""The float64 model of a top-k pass's start threshold (tests/seed_ref.py) on the CPU: its launch-side mirrors against hand-computed
cases, and the conditions on the planted corpora that the GPU test of the survivor counts (tests/test_seed_gpu.py) rests on.
These are conditions on the inputs, not measurements of the code under test."""
import contextlib
import math
import time

import numpy as np
import pytest

import seed_ref as sd
from seed_ref import with_parts


# ---- the launch side --------------------------------------------------------------------------------------------------------------------
def test_seed_plan_by_hand():
    """fill_params: seed_blocks = min(min(parts, 64) * 8, blocks of segment 0), shift = the largest with seed_blocks << shift <= blocks"""
    assert sd.seed_plan(3007, with_parts(1)) == (8, 3)       # 94 blocks: 8 << 3 = 64 <= 94 < 128; seed blocks 0, 8, ..., 56
    assert sd.seed_plan(3007, 0) == (94, 0)                  # min(512, 94): every block is a seed block
    assert sd.seed_plan(3007, with_parts(2)) == (16, 2)      # 16 << 2 = 64 <= 94 < 128
    assert sd.seed_plan(40_000, 0) == (512, 1)               # 1 250 blocks: 1 024 <= 1 250 < 2 048
    assert sd.seed_plan(20_000, with_parts(1)) == (8, 6)     # 625 blocks: 512 <= 625 < 1 024
    assert sd.seed_plan(400_000, 0) == (512, 4)              # 12 500 blocks: 8 192 <= 12 500 < 16 384
    assert sd.seed_plan(400_000, with_parts(255)) == (512, 4)  # the field is capped at kSeedParts
    assert sd.seed_plan(1, with_parts(1)) == (1, 0) and sd.seed_plan(31, 0) == (1, 0)
    assert sd.seed_plan(33, with_parts(1)) == (2, 0)         # two blocks, the second with one row
    assert sd.seed_plan(401, with_parts(1)) == (8, 0) and sd.seed_plan(401, 0) == (13, 0)  # 13 blocks: 16 > 13
    assert sd.seed_plan(3007, with_parts(1) | 0xFF00FFFF) == (8, 3)  # only bits 16..23 count
    # the sample: position sr -> row sr & 31 of block (sr >> 5) << shift, rows behind the segment's end left out
    sample, row = sd.seed_sample(3007, (8, 3))
    assert len(sample) == 256 and row[0] == 0 and row[31] == 31 and row[32] == 8 * 32 and row[255] == 56 * 32 + 31
    sample, row = sd.seed_sample(33, (2, 0))
    assert sample.tolist() == list(range(33)) and row.tolist() == list(range(33))
    sample, row = sd.seed_sample(3007, (94, 0))
    assert len(sample) == 3007 and (sample == row).all()


def test_seed_form_by_hand():
    """launch_prep_seed.  The MFMA seed needs 32 (Dp + 4) 4 + 32 k 4 bytes of the 156 KB (159 744 bytes): 139 776 + 128 k at
    Dp = 1088 — every k up to 128 fits; 147 968 + 128 k at 1 152 — k <= 92; 156 160 + 128 k at 1 216 — k <= 28; 164 352 at
    1 280 — never.  The boundaries are k = 92 | 93 and 28 | 29; k = 81 | 82 and 17 | 18 lie on the MFMA side of them."""
    for k in (1, 10, 128):
        assert sd.seed_form(32, 1088, k, 0) == "mfma" and sd.seed_form(32, 1280, k, 0) != "mfma"
    assert [sd.seed_form(32, 1152, k, 0) for k in (81, 82, 92, 93)] == ["mfma", "mfma", "mfma", "valu8"]
    assert [sd.seed_form(32, 1216, k, 0) for k in (17, 18, 28, 29)] == ["mfma", "mfma", "mfma", "valu8"]
    assert 147_968 + 128 * 92 <= 156 * 1024 < 147_968 + 128 * 93 and 156_160 + 128 * 28 <= 156 * 1024 < 156_160 + 128 * 29
    assert sd.seed_form(64, 128, 10, 0) == "mfma" and sd.seed_form(64, 128, 10, sd.FLAG_VALU_SEED) == "valu8"
    assert sd.seed_form(64, 128, 10, sd.FLAG_SEED16) == "mfma"                   # bit 1 alone changes nothing below 1 152 features
    assert sd.seed_form(2, 128, 10, sd.FLAG_VALU_SEED) == "valu1" and sd.seed_form(3, 128, 10, sd.FLAG_VALU_SEED) == "valu8"
    assert sd.seed_form(32, 1920, 10, 0) == "valu8" and sd.seed_form(32, 1984, 10, 0) == "valu1"  # 8 (Dp 4 + 512) <= 65 536 iff Dp <= 1 920
    assert sd.seed_form(32, 2496, 10, 0) == "valu1" and sd.seed_form(7, 2048, 32, 0) == "valu1" and sd.seed_form(5, 1536, 64, 0) == "valu8"
    both = sd.FLAG_SEED16 | sd.FLAG_VALU_SEED
    assert sd.seed_form(33, 896, 10, both) == "valu16" and sd.seed_form(32, 896, 10, both) == "valu8"
    assert sd.seed_form(64, 960, 10, both) == "valu8"                             # 16 (Dp 4 + 512) <= 65 536 iff Dp <= 896
    assert sd.seed_form(64, 1536, 10, both) == "valu8"


def test_guess_rank_by_hand():
    """choose_guess: the smallest j < k with C(k - 1, j) ratio^j < 1e-6, none from ratio = 0.25 on or for k < 2"""
    def slow(k, rows, seed_rows):
        ratio = seed_rows / rows
        if ratio >= 0.25:
            return None
        return next((j for j in range(1, k) if math.comb(k - 1, j) * ratio ** j < 1e-6), None)

    assert sd.guess_rank(10, 20_000, 256) == 5        # 126 * 0.0128^4 = 3.4e-6, 126 * 0.0128^5 = 4.3e-8
    assert sd.guess_rank(2, 20_000, 256) is None      # j = 1 alone: 0.0128
    assert sd.guess_rank(2, 10 ** 9, 256) == 1        # 2.56e-7
    assert sd.guess_rank(10, 400_000, 16_384) == 6
    assert sd.guess_rank(1, 10 ** 9, 256) is None and sd.guess_rank(128, 1024, 256) is None and sd.guess_rank(128, 1025, 256) is not None
    for k in (2, 3, 10, 100, 128):
        for rows, seed_rows in ((20_000, 256), (3007, 256), (40_000, 16_384), (10 ** 7, 16_384), (10 ** 8, 16_384)):
            assert sd.guess_rank(k, rows, seed_rows) == slow(k, rows, seed_rows), (k, rows, seed_rows)


def test_seed_slots_by_hand():
    """70 rows of 2-d under the dot metric, one query (1, 0): the score of row i is its first component.  parts = 1: three blocks,
    all seed blocks, sr = row; k = 4: slot j = the best of rows j, j + 4, ..."""
    x = np.zeros((70, 2), np.float32)
    x[:, 0] = np.arange(70) % 9 - 4.0
    x[:, 1] = 1.0
    x[68, 0] = np.inf        # no scale: not ranked
    x[17] = 0.0              # a zero row ranks with score 0 under the dot metric
    rows = sd.Rows(x, "dot")
    qs = sd.Queries(np.array([[1.0, 0.0]], np.float32), rows)
    plan = sd.seed_plan(70, with_parts(1))
    assert plan == (3, 0)
    want = [max(float(x[i, 0]) for i in range(j, 70, 4) if i != 68) for j in range(4)]
    slots = sd.seed_slots(rows, qs, 4, plan)
    np.testing.assert_array_equal(slots, [want])
    assert (sd.tau_start(slots, None) == min(want)).all() and (sd.tau_start(slots, 2) == sorted(want)[-2]).all()
    # more groups than seed rows: the groups without a row are -inf, and so is the threshold
    slots = sd.seed_slots(rows, qs, 100, plan)
    assert np.isinf(slots[0, 70:]).all() and np.isinf(sd.tau_start(slots, None)).all() and slots[0, 68] == -np.inf
    # the two faults: a row the seed does not see, a row ranked in another group
    best = int(np.argmax(np.where(np.arange(70) % 4 == 1, np.where(np.isfinite(x[:, 0]), x[:, 0], -9), -9)))
    lost = sd.seed_slots(rows, qs, 4, plan, drop=[best])
    assert lost[0, 1] <= want[1] and (np.delete(lost[0], 1) == np.delete(want, 1)).all()
    moved = sd.seed_slots(rows, qs, 4, plan, move=([best], [2]))
    assert moved[0, 2] == max(want[2], want[1]) and moved[0, 1] <= want[1]


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------------
def test_shapes_reach_every_form():
    reached = {}
    for s in sd.PINNED:
        assert sd.form_of(s) == s.form, s
        reached.setdefault(s.form, []).append(s)
    assert set(reached) == {"mfma", "valu1", "valu8", "valu16"}
    at = {(s.D, s.k): s.form for s in sd.PINNED if s.screen == "f32"}
    # both sides of the MFMA seed's LDS boundary, and two more pairs of k below it at either width
    assert at[(1152, 92)] == "mfma" and at[(1152, 93)] == "valu8" and at[(1216, 28)] == "mfma" and at[(1216, 29)] == "valu8"
    assert {(1152, 81), (1152, 82), (1216, 17), (1216, 18)} <= set(at)
    assert 1280 in {sd.padded(s.D) for s in reached["valu8"]} and all(sd.padded(s.D) >= 1280 for s in reached["valu1"] if s.screen == "f32")
    assert all(sd.seed_form(s.B, 1280, k, 0) != "mfma" for s in reached["valu8"] if s.D == 1280 for k in (1, s.k, sd.MAX_K))
    # the widest rows each form takes: P = 144 and 152 pieces per lane in the MFMA seed, 2 496 features in the one-query form
    assert {1152, 1216} <= {s.D for s in reached["mfma"]} and 2496 in {s.D for s in reached["valu1"]} and 2048 in {s.D for s in reached["valu1"]}
    assert {(s.D, s.B) for s in reached["valu8"]} >= {(1280, 32), (1536, 5), (1536, 32), (128, 8)}
    assert {(s.D, s.B) for s in reached["valu1"]} >= {(128, 1), (128, 2), (2048, 7), (2496, 32)}
    assert {(s.D, s.B) for s in reached["valu16"]} == {(D, B) for D in (384, 896) for B in (33, 64)}
    assert all(s.flags & 6 == 6 for s in reached["valu16"])
    assert {(s.D, s.B) for s in reached["mfma"]} >= {(128, 8), (128, 64), (1152, 32), (1216, 32)}
    # the seed stride: one part on 94 blocks, and one shape at the default 64 parts
    plans = {sd.seed_plan(s.rows, s.flags) for s in sd.PINNED}
    assert plans == {(8, 3), (512, 1)}
    for s in sd.PINNED + sd.GUESS:
        assert 3000 <= s.rows <= 40_000 and s.k <= sd.MAX_K
        sd.scan_of(s)  # one pass: scan_form asserts that the pass takes B queries
        if s.screen != "wave":
            assert s.B <= (sd.sr.mfma8_pass_queries(sd.padded(s.D)) if s.screen == "int8" else sd.sr.mfma_pass_queries(sd.padded(s.D)))
    assert all(s.flags & sd.FLAG_NO_GUESS for s in sd.PINNED) and all(s.flags & sd.FLAG_NO_LEARNED and not s.flags & sd.FLAG_NO_GUESS for s in sd.GUESS)
    # the wave shapes, and the two copies of the mid test's reader
    assert {type(sd.scan_of(s)).__name__ for s in sd.PINNED} >= {"Drain", "Mfma", "Wave"}
    assert {(s.D, s.screen, s.B, s.k) for s in sd.GUESS} == {(D, sc, B, k) for D, sc in ((128, "int8"), (640, "bf16")) for B in (5, 64) for k in (2, 10, 128)}


PINNED_IDS = [f"{s.form}-{s.D}d-B{s.B}-k{s.k}-{s.rows}" for s in sd.PINNED]
GUESS_IDS = [f"{s.screen}-{s.D}d-B{s.B}-k{s.k}" for s in sd.GUESS]


@pytest.mark.parametrize("metric", sd.METRICS)
@pytest.mark.parametrize("shape", sd.PINNED, ids=PINNED_IDS)
def test_pinned_cases_are_pinned(shape, metric):
    """the construction: every query's k best rows are seed rows, one in each seed group; min(slots) is the k-th best score, every
    slot is a planted row of the query's cluster, and no other row with a score comes within GAP eps32 unit of the k-th"""
    c = sd.Pinned.get(shape, metric)
    sample, srow = sd.seed_sample(shape.rows, c.plan)
    group = dict(zip(srow.tolist(), (sample % shape.k).tolist()))
    s = sd.scores64(c.rows, c.qs)[: shape.rows]
    s = np.where(np.isfinite(s) & (c.rows.scale[: shape.rows] != 0)[:, None], s, -np.inf)
    for b in range(shape.B):
        mine = c.planted[c.cluster[b]]
        assert sorted(group[int(r)] for r in mine) == list(range(shape.k))
        order = np.argsort(-s[:, b], kind="stable")
        assert set(order[: shape.k].tolist()) == set(mine.tolist())
        np.testing.assert_array_equal(np.sort(c.slots[b]), np.sort(s[mine, b]))
        assert c.tau[b] == c.kth[b] == s[mine, b].min()
        assert s[order[shape.k], b] < c.kth[b] - c.GAP * sd.eps32(shape.D) * c.qs.unit[b]
    # the planted rows lie over the whole sample: every eighth of it (at one seed part: every seed block) holds some
    at = dict(zip(srow.tolist(), sample.tolist()))
    eighths = {at[int(r)] * 8 // (c.plan[0] * 32) for r in c.planted.reshape(-1)}
    assert eighths == set(range(8)), eighths
    assert c.rows.scale[c.zero_row] == 0 or metric == "dot"
    assert c.rows.nonfinite[c.inf_row] and c.inf_row in group and c.zero_row in group
    # the clusters' thresholds differ by far more than a bracket is wide: a threshold read for another query moves the counts
    if c.G > 1:
        rel = c.tau / c.qs.unit
        assert np.abs(rel[: c.G, None] - rel[None, : c.G])[~np.eye(c.G, dtype=bool)].min() > 0.005


@pytest.mark.parametrize("metric", sd.METRICS)
@pytest.mark.parametrize("shape", sd.PINNED, ids=PINNED_IDS)
def test_pinned_brackets_are_tight_and_have_teeth(shape, metric):
    """What test_seed_gpu.py rests on.  coarse_survivors and mid_survivors: the bracket is at most 2 % wide and holds at least 200
    rows, the condition of test_screens_cpu.py.  candidates: the fine test's margin (2 eps32 unit) is the size of e itself, so a
    row is a candidate at both ends of the bracket only if it is 0.7 eps32 unit or more above the k-th best score — the other
    k - 1 planted rows — and at the high end only if it is within some 5 eps32 unit below it, where the construction has the k-th
    row alone: the bracket is B (k - 1) .. B k, one row per query wide, and cannot be tighter without a row that ties the k-th.
    Teeth: with one seed group lost (the k-th planted row unseen) and with two planted rows in one group, the threshold falls to
    that group's next best seed row, and every count the pass reports — every test tightened — lies above its bracket."""
    c = sd.Pinned.get(shape, metric)
    br = c.bracket()
    print(f"D={shape.D} {metric} B={shape.B} k={shape.k} {shape.form} plan={c.plan} clusters={c.G}: "
          + ", ".join(f"{name} {lo} .. {hi} ({100.0 * (hi - lo) / hi:.2f} %)" for name, (lo, hi) in br.items()))
    assert set(br) == ({"candidates"} if shape.screen == "wave" else {"coarse", "candidates", "mid"} if shape.mid == "on" else {"coarse", "candidates"})
    assert br["candidates"] == (shape.B * (shape.k - 1), shape.B * shape.k)
    for name, (lo, hi) in br.items():
        if name != "candidates":
            assert lo >= 200, (name, lo)
            assert hi - lo <= 0.02 * hi, (name, lo, hi)
    if "coarse" in br:
        assert br["coarse"][0] >= shape.B * shape.k + 100  # not the planted rows alone: ladder rows inside the band
    for fault in ("lost", "shared"):
        tau, got = c.faulty(fault)
        assert (tau < c.tau - c.GAP * sd.eps32(shape.D) * c.qs.unit).all()
        print(f"    {fault}: " + ", ".join(f"{name} {v}" for name, v in got.items()))
        for name, (lo, hi) in br.items():
            assert got[name] > hi + max(50, 0.1 * hi), (fault, name, got[name], hi)


@pytest.mark.parametrize("metric", sd.METRICS)
@pytest.mark.parametrize("shape", sd.GUESS, ids=GUESS_IDS)
def test_guess_bound_means_something(shape, metric):
    """the k best rows of every query lie outside the seed blocks and clear the start threshold by more than margin32 + eps32 unit
    (rescore_select_kernel wants k rows at guess + margin32); where there is a guess, the high end of every count at the guess is
    at most half the low end at min(slots) — a pass whose guess was silently not applied starts from there.  k = 2 has no guess
    at 20 000 rows (C(1, 1) 256 / 20 000 > 1e-6): the pass starts from min(slots), and the bound is the one at min(slots)."""
    c = sd.Guess.get(shape, metric)
    assert c.plan == (8, 6) and c.rank == {2: None, 10: 5, 128: 12}[shape.k]
    qs, slots, tau, lowest = c.run(shape)
    seed_block = ((c.planted[: shape.B] >> 5) & 63) == 0
    assert not (seed_block & ((c.planted[: shape.B] >> 5) >> 6 < 8)).any()
    s = sd.scores64(c.rows, qs)[: shape.rows]
    m32 = sd.margins(c.rows, qs)[1]
    for b in range(shape.B):
        order = np.argsort(-np.where(np.isfinite(s[:, b]), s[:, b], -np.inf), kind="stable")
        assert set(order[: shape.k].tolist()) == set(c.planted[b].tolist())
        assert s[c.planted[b], b].min() > tau[b] + 10 * (m32[b] + sd.eps32(shape.D) * qs.unit[b])
    hi, lo = c.high(shape), c.low_without(shape)
    print(f"D={shape.D} {metric} B={shape.B} k={shape.k} rank={c.rank}: " + ", ".join(f"{n} <= {hi[n]} (without the guess >= {lo[n]})" for n in hi))
    if c.rank is None:
        assert (tau == lowest).all()
    else:
        assert (tau > lowest).all()
        for name in hi:
            assert 2 * hi[name] <= lo[name], (name, hi[name], lo[name])


def _least_of_three(run):
    took = []
    while len(took) < 3 and (not took or min(took) >= 0.5):
        t = time.perf_counter()
        run()
        took.append(time.perf_counter() - t)
    return took


def test_the_model_is_quick():
    """the float64 model of the largest shapes — the widest rows (3 007 x 2 496, the f32 screen), the most rows (40 000 x 128,
    64 queries, the int8 screen) and the most numbers (the guess case of 20 000 x 640, 64 queries, k = 128) — stays under a second
    each: rows, queries, slots and counts, from the arrays alone.  Other work on the machine only ever adds to a wall-clock time,
    so the figure is the least of up to three runs of the same work.  The model's products are skinny (n x D by D x B): BLAS
    threads gain nothing on them, and a pool that has just been woken takes the cores from numpy's own loops, so the runs take
    one BLAS thread where threadpoolctl is there."""
    try:
        from threadpoolctl import threadpool_limits
        one_thread = threadpool_limits(limits=1, user_api="blas")
    except ImportError:
        one_thread = contextlib.nullcontext()
    shapes = [max(sd.PINNED, key=lambda s: s.D), max(sd.PINNED, key=lambda s: s.rows), max(sd.GUESS, key=lambda s: (s.rows * s.D, s.B, s.k))]
    assert [(s.rows, s.D, s.B) for s in shapes] == [(3007, 2496, 32), (40_000, 128, 64), (20_000, 640, 64)]
    assert all(s.rows * s.D <= shapes[2].rows * shapes[2].D for s in sd.PINNED + sd.GUESS)
    for shape in shapes:
        guess = shape in sd.GUESS
        c = (sd.Guess if guess else sd.Pinned).get(shape, "cosine")
        out = []

        def run():
            rows = sd.Rows(c.corpus, "cosine")
            qs = sd.Queries(c.queries[: shape.B], rows)
            slots = sd.seed_slots(rows, qs, shape.k, c.plan)
            if guess:
                out.append(sd.counts([rows], qs, sd.tau_start(slots, c.rank), shape.screen, None, shape.D, 1.0, sd.eps32(shape.D) * qs.unit))
            else:
                out.append(sd.bracket([rows], qs, sd.tau_start(slots, None), shape.screen, sd.mid_of(shape), shape.D))

        with one_thread:
            took = _least_of_three(run)
        assert out[-1] == (c.high(shape) if guess else c.bracket())
        print(f"{shape.rows} x {shape.D}, {shape.B} queries: " + ", ".join(f"{v:.2f} s" for v in took))
        assert min(took) < 1.0
