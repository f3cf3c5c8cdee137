"""GPU: every scan screen's survivor counts against the float64 model of tests/screens_ref.py, kernel form by kernel form.

A range pass fixes its thresholds before the scan and nothing raises them (range_thresholds_kernel; DESIGN.md §4 "Range search"),
so the rows its screens let through — coarse_survivors, mid_survivors, candidates — are a function of the copies and the query
constants alone.  Final hits cannot see a screen that is too loose (it only costs time) and see one that is too tight only when a
true hit lies in the missing sliver; the counts see both.  Each shape of screens_ref.SHAPES is one pass over 3 007 rows (a 31-row
last block, an all-zero row, a row with an inf, a row with one dominant component), selected with set_screening_copy,
set_mid_copy, set_kernel and set_tuning; a shape with more than one 32-query tile is run again once per tile with the other
tiles' bounds admitting nothing, so that a threshold read for the wrong query, tile or half moves a count from hundreds to
nothing or back.  tests/test_screens_cpu.py holds every bracket used here to 2 % and at least 200 rows, and checks that the
shapes reach every form the launchers can choose."""
import numpy as np
import pytest

import perceive_amd as pa
import screens_ref as sr

pytestmark = pytest.mark.gpu

COPY = {"int8": ("int8", 2, 8), "bf16": ("bf16", 1, 0), "f32": ("off", 0, 0), "wave": ("off", 0, 0)}  # set_screening_copy, screening_copy, screen_bits


def build(ctx, case, shape):
    s = pa.Searcher(ctx, case.D, case.metric)
    s.set_tuning(shape.flags)
    s.set_screening_copy(COPY[shape.screen][0])
    s.set_mid_copy(shape.mid)
    if shape.screen == "f32":
        s.set_kernel("mfma")  # (AUTO takes the wave kernel for up to four queries without a copy)
    for i, (a, b) in enumerate(zip(case.cuts[:-1], case.cuts[1:])):
        s.add_rows(i + 1, case.corpus[a:b], np.arange(a, b, dtype=np.int64))  # ids: the oracle's positions
        s.finalize()
    assert s.num_segments == len(case.cuts) - 1 and s.num_rows == len(case.corpus)
    return s


def one_pass(s, case, shape, tile):
    B = shape.B
    bounds = case.bounds(B, tile)
    ids, scores, counts, more = s.search_range(None, bounds, case.queries[:B], 256)
    st = s.last_stats()
    want = case.bracket(shape, tile)
    names = {"coarse": "coarse_survivors", "mid": "mid_survivors", "candidates": "candidates"}
    print(f"D={case.D} {case.metric} {shape.group} B={B} flags={shape.flags:#x} {sr.form_of(shape)} tile={tile}: "
          + ", ".join(f"{k} {st[names[k]]} (model {lo} .. {hi})" for k, (lo, hi) in want.items()))
    assert st["scan_launches"] == 1
    assert st["screening_copy"] == COPY[shape.screen][1] and st["screen_bits"] == COPY[shape.screen][2]
    assert st["mid_copy"] == (1 if shape.mid == "on" else 0)
    inr = case.in_range(B, tile)
    np.testing.assert_array_equal(counts, inr)
    assert not more.any()
    for q in range(B):
        m = int(inr[q])
        np.testing.assert_array_equal(ids[q, :m], case.opos[q, :m])
        np.testing.assert_allclose(scores[q, :m], case.orep[q, :m], rtol=0, atol=1e-7)
    for k, (lo, hi) in want.items():
        assert lo <= st[names[k]] <= hi, (k, st[names[k]], lo, hi)
    if shape.mid != "on":
        assert st["mid_survivors"] == 0


def run_group(ctx, oracle, group, D, metric):
    shapes = [s for s in sr.SHAPES if s.group == group and s.D == D]
    assert shapes
    searchers = {}
    try:
        for shape in shapes:
            case = sr.case_of(oracle, shape, metric)
            key = (shape.screen, shape.mid, shape.segs)
            if key not in searchers:
                searchers[key] = build(ctx, case, shape)
            s = searchers[key]
            s.set_tuning(shape.flags)
            tiles = sr.tiles_of(shape)
            for tile in [None] + (list(range(tiles)) if tiles > 1 else []):
                one_pass(s, case, shape, tile)
    finally:
        for s in searchers.values():
            s.close()


def dims(group):
    return sorted({s.D for s in sr.SHAPES if s.group == group})


@pytest.mark.parametrize("metric", sr.METRICS)
@pytest.mark.parametrize("D", dims("drain"))
def test_int8_drain_form(ctx, oracle, D, metric):
    """scan_mfma8_kernel<NT, NTL, 12, NBUF, true, NCHT>: 5, 32, 33 and 64 queries at every chunk count, the two run-time ones
    (640-d, 896-d) included; three chunk buffers and plain loads where SHAPES has them"""
    run_group(ctx, oracle, "drain", D, metric)


@pytest.mark.parametrize("metric", sr.METRICS)
@pytest.mark.parametrize("D", dims("four"))
def test_int8_four_wave_form(ctx, oracle, D, metric):
    """one and four queries, and kFlagFourWave at 16 and 64: every wave takes its own survivors through fine_survivors"""
    run_group(ctx, oracle, "four", D, metric)


@pytest.mark.parametrize("metric", sr.METRICS)
@pytest.mark.parametrize("D", dims("tile128"))
def test_int8_128_query_tile(ctx, oracle, D, metric):
    """above 384 features (two tiles a CU at 512-d, eight waves on one at 768-d) and under kFlagTile128"""
    run_group(ctx, oracle, "tile128", D, metric)


@pytest.mark.parametrize("metric", sr.METRICS)
@pytest.mark.parametrize("D", dims("hold"))
def test_int8_hold_kernel(ctx, oracle, D, metric):
    """scan_mfma8_hold_kernel at two and four halves, full and partial, with non-temporal and plain loads: every tile's U on its own"""
    run_group(ctx, oracle, "hold", D, metric)


@pytest.mark.parametrize("metric", sr.METRICS)
@pytest.mark.parametrize("D", dims("mid"))
def test_mid_test_in_both_copies(ctx, oracle, D, metric):
    """fine_survivors (4, 100, 256 queries) and drain_survivors (64) read the mid copy: mid_survivors against keep_mid"""
    run_group(ctx, oracle, "mid", D, metric)


@pytest.mark.parametrize("metric", sr.METRICS)
@pytest.mark.parametrize("D", dims("bf16"))
def test_bf16_copy(ctx, oracle, D, metric):
    run_group(ctx, oracle, "bf16", D, metric)


@pytest.mark.parametrize("metric", sr.METRICS)
@pytest.mark.parametrize("D", dims("f32rows"))
def test_f32_rows_through_the_mfma_kernel(ctx, oracle, D, metric):
    """no copy: the loop converts v * scale, and the row with an inf is a coarse survivor of every query (screens_ref.keep_bf16)"""
    run_group(ctx, oracle, "f32rows", D, metric)


@pytest.mark.parametrize("metric", sr.METRICS)
@pytest.mark.parametrize("D", dims("wave"))
def test_wave_kernel(ctx, oracle, D, metric):
    run_group(ctx, oracle, "wave", D, metric)


@pytest.mark.parametrize("metric", sr.METRICS)
def test_several_segments(ctx, oracle, metric):
    """seven segments of 1 to 900 rows: a SegCursor change inside a wave's stream, in the drain form and the four-half hold kernel"""
    run_group(ctx, oracle, "segments", 200, metric)
