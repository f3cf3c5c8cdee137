"""CPU: the float64 model of the row-pair screens (pairs_ref.py) is sound, and the cases test_pairs_gpu.py runs are tight.

  - every run's bracket is non-trivial: lo >= 200 and (hi - lo) <= cap * lo, cap = 0.02 for the fixed-threshold screens at Dp <= 768
    and 0.05 for the others (Run.cap).  For a tree the bracket of the call — the sum over its rounds, what stats["candidates"]
    holds — is held to this; the late rounds of a tree list too few pairs for a cap of their own, and test_pairs_gpu.py holds every
    round to its bracket whatever its width;
  - a simulated screen (the model's scores plus f32 noise of the slack's size) stays inside every bracket, and leaves the bracket of
    at least one run once a fault is built into it;
  - the mirrors of the host's choices (neighbor_sample, the trees' stride, the tile size, the margin) against hand-computed values."""
import functools

import numpy as np
import pytest

import pairs_ref as pr
from density_ref import margin as density_margin


@functools.lru_cache(maxsize=None)
def bracket(i):
    return pr.bracket(pr.RUNS[i])


@functools.lru_cache(maxsize=2)
def device(key, select, fault):
    """a simulated device over the corpus of a run (the model's own Corpus: it is read only)"""
    m = pr.Model(pr.model(key, select).c, simulate=3, fault=fault)
    return m if m.c.L > 4096 else m.dense()


def simulated(r, fault=None, **rule):
    return pr.bracket(r, device(r.key, r.select, fault), **rule)


def outside(r, want, got):
    """the brackets of `want` that the counts of `got` leave (a simulated screen's are a point, or two counts a rounding of a
    threshold apart)"""
    return [(name, lo, hi, g, g2) for (name, lo, hi), (_n, g, g2) in zip(pr.brackets_of(r, want), pr.brackets_of(r, got)) if not lo <= g <= g2 <= hi]


RUN_IDS = [pr.run_id(r) for r in pr.RUNS]


@pytest.mark.parametrize("i", range(len(pr.RUNS)), ids=RUN_IDS)
def test_bracket_is_narrow_and_holds_a_sound_screen(i):
    r = pr.RUNS[i]
    b = bracket(i)
    c = pr.model(r.key, r.select).c
    for name, lo, hi in pr.brackets_of(r, b):
        print("%s %s: %d .. %d (%.2f %%)" % (RUN_IDS[i], name, lo, hi, 100.0 * (hi - lo) / max(lo, 1)))
        assert 0 <= lo <= hi
        if not name.startswith("round"):
            assert lo >= 200 and hi - lo <= r.cap * lo
    if r.grows:  # the list outgrows its first room, whatever the device's rounding does
        cap = pr.first_capacity(r, c)
        per_list = [x for x in pr.brackets_of(r, b) if x[0].startswith("round")] if r.screen in ("linkage", "reach") else pr.brackets_of(r, b)[-1:]
        assert any(lo > cap for _n, lo, _hi in per_list) and not any(lo <= cap < hi for _n, lo, _hi in per_list)
    if r.screen in ("linkage", "reach"):
        rounds = (b[1] if r.screen == "reach" else b).rounds
        assert rounds[0].before == c.P and rounds[-1].after == 1 and all(x.after == y.before for x, y in zip(rounds, rounds[1:]))
    # the simulated device: inside every bracket, the rounds' too
    assert outside(r, b, simulated(r)) == []


def first(screen, key, *args):
    return next(i for i, r in enumerate(pr.RUNS) if (r.screen, r.key, r.args[: len(args)]) == (screen, key, args) and r.select is None)


# (fault, the runs it is tried on, the score fault, the rule fault): every fault must leave the bracket of one of its runs
FAULTS = [
    ("the margin doubled", [("join", "g384"), ("density", "g64"), ("neighbors", "g384", 10), ("assign", "g384", 300)], None, {"margin_scale": 2.0}),
    ("m where 2 m belongs in the neighbour threshold", [("neighbors", "g384", 10)], None, {"margins": 1.0}),
    ("m where 2 m belongs in the linkage threshold", [("linkage", "g384")], None, {"margins": 1.0}),
    ("s moved by 1e-3", [("join", "g64"), ("density", "g384")], "shift", {}),
    ("the rb of block g + 1 used for block g", [("join", "g64"), ("neighbors", "g384", 10)], "rb_next", {}),
    ("the accumulator of a block not cleared", [("join", "g384"), ("linkage", "g64")], "stale_acc", {}),
    ("the diagonal rule dropped", [("join", "g384"), ("density", "g640")], None, {"diagonal": False}),
    ("the assign bound not carried from tile to tile", [("assign", "g384", 300), ("assign", "g640", 300)], None, {"carry": False}),
    ("the reach cap ignored in the list pass", [("reach", "g384", 16), ("reach", "g64", 5)], None, {"cap_list": False}),
]


@pytest.mark.parametrize("what, where, fault, rule", FAULTS, ids=[f[0] for f in FAULTS])
def test_a_faulty_screen_leaves_a_bracket(what, where, fault, rule):
    caught = []
    for spec in where:
        i = first(*spec)
        r = pr.RUNS[i]
        out = outside(r, bracket(i), simulated(r, fault, **rule))
        print("%s on %s: %s" % (what, RUN_IDS[i], out or "inside"))
        caught += out
    assert caught, what
    # ... and on every one of them, not on one alone, for the faults of a rule that every call runs through
    if fault is None and "margin" in what:
        assert all(outside(pr.RUNS[first(*s)], bracket(first(*s)), simulated(pr.RUNS[first(*s)], fault, **rule)) for s in where)


def test_mirrors_against_hand_computed_values():
    # neighbor_sample(TB, k) -> (stride, span_len, spans): stride = min(4, max(1, TB / max(64, 4 k))); the sampled blocks in
    # min(sampled, 512, max(64, 8 k)) spans of equal length, the last one shorter
    assert pr.neighbor_sample(94, 10) == (1, 2, 47)    # 94 sampled, 80 wanted: spans of 2
    assert pr.neighbor_sample(94, 1) == (1, 2, 47)     # 64 wanted: spans of 2
    assert pr.neighbor_sample(94, 64) == (1, 1, 94)    # 512 wanted, 94 there are
    assert pr.neighbor_sample(385, 10) == (4, 2, 49)   # 385 / 64 = 6 -> 4; 97 sampled, 80 wanted
    assert pr.neighbor_sample(385, 64) == (1, 1, 385)  # 385 / 256 = 1
    assert pr.neighbor_sample(2048, 64) == (4, 1, 512)
    assert pr.neighbor_sample(3, 5) == (1, 1, 3)
    assert [pr.linkage_stride(tb) for tb in (1, 63, 64, 94, 127, 128, 255, 256, 385)] == [1, 1, 1, 1, 1, 2, 3, 4, 4]
    assert [pr.join_spans(tb) for tb in (94, 256, 257, 385)] == [1, 1, 2, 2]
    # the tile: 128 / 64 / 32 rows for Dp <= 576 / <= 1216 / above, none above 2496 (156 KB of LDS, 2 bytes a feature)
    assert [pr.tile_rows(d) for d in (1, 64, 576, 577, 640, 1216, 1217, 1280, 2496, 2497)] == [128, 128, 128, 64, 64, 64, 32, 32, 32, 0]
    assert [pr.padded(d) for d in (1, 50, 64, 65, 130)] == [64, 64, 64, 128, 192]
    # selfjoin_margin: 0.00783 + 1.02 (Dp + 16) 1.2e-7 + 1e-6
    for d in (64, 384, 1280):
        assert abs(pr.margin(d) - (0.00783 + 1.02 * (d + 16) * 1.2e-7 + 1e-6)) < 1e-9 and pr.margin(d) == density_margin(d)
        assert pr.slack(d) < pr.margin(d) / 40  # the screen's own error is a small part of what the margin certifies
    assert pr.screen_threshold(0.5, 64) < 0.5 - pr.margin(64) <= float(np.nextafter(np.float32(pr.screen_threshold(0.5, 64)), np.float32(1)))
    lo, hi = pr.density_thresholds(0.5, 64)
    assert lo < 0.5 - pr.margin(64) and hi > 0.5 + pr.margin(64) and hi - lo < 2 * pr.margin(64) + 3e-7
    assert pr.f32_down(0.1) < 0.1 < pr.f32_up(0.1) and pr.f32_down(0.5) == pr.f32_up(0.5) == 0.5


def test_rinv_and_layout():
    rows = np.ones((70, 64), dtype=np.float32)
    rows[3] = 0.0
    rows[4] *= np.float32(2.0 ** -24)   # |x|^2 = 2^-42: below 2^-40
    rows[5] *= np.float32(2.0 ** 18)    # |x|^2 = 2^42
    rows[6] *= np.float32(2.0 ** -66)   # |x|^2 = 2^-126: the least with a cosine
    rows[7] *= np.float32(2.0 ** -67)
    hidden = np.zeros(70, dtype=bool)
    hidden[8] = True
    c = pr.Corpus(rows, [np.arange(0, 33), np.arange(33, 70)], hidden)
    assert c.L == 128 and c.TB == 4 and c.rows_selected == 70
    assert (c.src[:33] == np.arange(33)).all() and (c.src[33:64] == -1).all() and c.src[64] == 33 and (c.src[101:] == -1).all()
    assert c.rinv[0] == np.float32(0.125) and c.rinv[3] == 0 and c.rinv[4] == -1 and c.rinv[5] == -1 and c.rinv[6] == -1 and c.rinv[7] == 0
    assert c.rinv[8] == 0 and (c.rinv[33:64] == 0).all() and c.rinv[64] == np.float32(0.125) and c.P == 70 - 3
    m = pr.Model(c)
    Slo, Shi = m.rows(0, 128)
    assert np.isnan(Slo[0, 3]) and np.isnan(Slo[4, 0]) and Slo[0, 1] < 1.0 < Shi[0, 1] and Shi[0, 1] - Slo[0, 1] <= 2 * pr.slack(64)
    # every pair of these identical rows is listed; the wild rows list every defined pair, rows without rinv nothing
    assert pr.join(m, 0.99) == (67 * 66 // 2,) * 2
    assert pr.neighbors(m, 1) == (67 * 66,) * 2
