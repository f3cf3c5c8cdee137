"""The float64 model of the scan screens (tests/screens_ref.py) on the CPU: its certificates on rows chosen to quantise badly,
the width of the brackets the GPU test of the survivor counts (tests/test_screens_gpu.py) rests on, and that the GPU test's
shapes reach every kernel form the launchers can choose."""
import zlib

import numpy as np
import pytest

import screens_ref as sr
import six_ref
from test_six_bound import adversarial_rows

WIDTHS = [64, 100, 200, 384, 640, 768, 1024]


# ---- certificates ---------------------------------------------------------------------------------------------------------------------
def half_step_rows(rng, D, count):
    """rows whose int8 and mid codes sit half a unit in the last place either side of a rounding boundary: one component is the
    row's largest (1), the others (k + 0.5) / 127 moved one f32 step up or down"""
    k = rng.integers(-126, 126, (count, D))
    v = ((k + 0.5) / 127.0).astype(np.float32)
    v = np.where(rng.random((count, D)) < 0.5, np.nextafter(v, np.float32(2.0)), np.nextafter(v, np.float32(-2.0)))
    v[np.arange(count), rng.integers(0, D, count)] = 1.0
    return v.astype(np.float32)


def certificate_case(oracle, D, metric):
    rng = np.random.default_rng(700 + D)
    x = adversarial_rows(rng, D, metric)  # 34 blocks: Cauchy rows (one dominant component), one-hot rows, rows on one step, ...
    x[128:192] = half_step_rows(rng, D, 64) * (1.0 if metric == "cosine" else 3.0)
    x = x[:-17]                                # a last block of 15 rows
    n = len(x)
    searchable = rng.random(n) > 0.1
    searchable[96:128] = False                 # block 3: no searchable row
    x[40] = 0.0                                # a zero row
    x[41, 5] = np.inf                          # a row with an inf
    x[300] *= np.float32(0.01)
    x[300, 0] = 20.0                           # one component far above the rest of its block
    searchable[[40, 41, 300]] = True
    rows = sr.Rows(x, metric, searchable)
    assert n % 32 == 15 and np.isnan(rows.s_blk[3]) and rows.nonfinite[41] and rows.scale[41] == 0
    queries = np.concatenate([rng.standard_normal((6, D)), rng.standard_cauchy((4, D)), x[:6], np.eye(D)[:2]]).astype(np.float32)
    qs = sr.Queries(queries, rows)
    # the oracle's canonical score of every row that has one
    pos, sc, cnt = oracle.topk(queries, x, n, metric=1 if metric == "dot" else 0)
    c = np.full((rows.nblk * 32, len(queries)), -np.inf)
    for q in range(len(queries)):
        c[pos[q, : cnt[q]], q] = sc[q, : cnt[q]]
    return rows, qs, c


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("D", WIDTHS)
def test_certificates_hold(oracle, D, metric):
    """No screen, tightened by its slack, drops a searchable row whose canonical score (the oracle's) is at or above the
    threshold: tau = each query's 98th percentile over the searchable rows, so hundreds of pairs stand above it."""
    rows, qs, c = certificate_case(oracle, D, metric)
    ok = rows.live[:, None] & np.isfinite(c)
    tau = np.array([np.quantile(c[ok[:, q], q], 0.98) for q in range(qs.B)])
    above = ok & (c >= tau[None, :])
    assert above.sum() >= 10 * qs.B
    sl = sr.slacks(D)
    screens = {
        "int8": sr.keep_int8(rows, qs, tau, -sl["int8"]),
        "bf16": sr.keep_bf16(rows, qs, tau, -sl["bf16"]),
        "f32 rows": sr.keep_bf16(rows, qs, tau, -sl["f32"], f32_rows=True),
        "mid": sr.keep_mid(rows, qs, tau, -sl["mid"]),
        "mid, 64 lanes": sr.keep_mid(rows, qs, tau, -sr.mid_slack(D, "fine_survivors")),
        "fine": sr.keep_fine(rows, qs, tau, -sl["fine"]),
    }
    for name, keep in screens.items():
        assert keep[above].all(), f"{name}: {(~keep[above]).sum()} pairs at or above tau dropped"
    # what the models say of the rows that are not searched
    assert not screens["int8"][96:128].any() and not screens["mid"][96:128].any() and not screens["fine"][~rows.live].any()
    np.testing.assert_array_equal(screens["f32 rows"][41], np.ones(qs.B, bool))     # NaN accumulators: kept by the coarse test
    np.testing.assert_array_equal(screens["bf16"][41], tau - sr.margins(rows, qs)[0] <= 0)  # zeros in the copy
    np.testing.assert_array_equal(screens["bf16"][rows.n :], np.broadcast_to(tau - sr.margins(rows, qs)[0] <= 0, (17, qs.B)))
    # slack: positive loosens, negative tightens, both nest round the test itself
    for fn, key in ((sr.keep_int8, "int8"), (sr.keep_bf16, "bf16"), (sr.keep_mid, "mid"), (sr.keep_fine, "fine")):
        lo, mid, hi = fn(rows, qs, tau, -sl[key]), fn(rows, qs, tau), fn(rows, qs, tau, sl[key])
        assert (lo <= mid).all() and (mid <= hi).all()


def test_keeps_uses_the_one_int8_test():
    rng = np.random.default_rng(3)
    rows = sr.Rows(rng.standard_normal((200, 100)).astype(np.float32), "cosine")
    qs = sr.Queries(rng.standard_normal((7, 100)).astype(np.float32), rows)
    tau = np.full(7, 0.1)
    for slack in (0.0, -1e-4, 1e-4):
        six, both = six_ref.keeps(rows, qs, tau, slack)
        np.testing.assert_array_equal(both, six & sr.keep_int8(rows, qs, tau, slack))
    assert sr.keep_int8 is six_ref.keep_int8


def test_range_case_draws_what_it_drew():
    """six_ref.range_case grew arguments; its defaults must give test_six_paths_gpu.py the inputs it had (CRC-32 of the rows and
    queries, recorded before the change)."""
    want = {(100, "cosine"): 0x30663F73, (100, "dot"): 0xA60CDD1C, (200, "cosine"): 0xAE5C698F, (200, "dot"): 0x9E97E87D,
            (384, "cosine"): 0xA3978AFA, (384, "dot"): 0xD1B542A3}
    for (D, metric), crc in want.items():
        assert drawn_crc(D, metric) == crc, (D, metric, hex(drawn_crc(D, metric)))


def drawn_crc(D, metric):
    class Stop(Exception):
        pass

    class Recorder:
        def topk(self, queries, corpus, k, metric=0):
            self.crc = zlib.crc32(corpus.tobytes(), zlib.crc32(queries.tobytes()))
            raise Stop

    rec = Recorder()
    saved = dict(six_ref._range_cases)
    try:
        six_ref._range_cases.clear()
        six_ref.range_case(rec, D, metric)
    except Stop:
        pass
    finally:
        six_ref._range_cases.clear()
        six_ref._range_cases.update(saved)
    return rec.crc


# ---- brackets -------------------------------------------------------------------------------------------------------------------------
def groups():
    seen = []
    for s in sr.SHAPES:
        if (s.D, s.segs, s.mid) not in seen:
            seen.append((s.D, s.segs, s.mid))
    return seen


@pytest.mark.parametrize("metric", sr.METRICS)
@pytest.mark.parametrize("D,segs,mid", groups())
def test_brackets_are_tight(oracle, D, segs, mid, metric):
    """The condition test_screens_gpu.py rests on, for every pass it runs — each shape whole, and each of its 32-query tiles on
    its own with the other tiles' bounds admitting nothing: the model's counts with every test tightened by its slack and with
    every test loosened by it differ by at most 2 % of the looser one (the cap of test_six_bound.py::test_model_bracket_is_tight),
    and the tightened count is at least 200 — a device count inside the bracket is then within 2 % of the model's, and one that
    fell to nothing, or doubled, is far outside.  The slacks are derived in screens_ref from the kernels' roundings."""
    case = sr.Case.get(oracle, D, metric, segs, blocks=mid == "on")
    done = set()
    for shape in sr.SHAPES:
        if (shape.D, shape.segs, shape.mid) != (D, segs, mid) or (shape.B, shape.screen, shape.mid) in done:
            continue
        done.add((shape.B, shape.screen, shape.mid))
        tiles = sr.tiles_of(shape)
        inr = case.in_range(shape.B)
        assert (inr >= 20).all() and (inr < sr.DEPTH).all() and (inr[case.kinds(shape.B) == sr.RANK] < 200).all()
        for tile in [None] + (list(range(tiles)) if tiles > 1 else []):
            br = case.bracket(shape, tile)
            print(f"D={D} {metric} B={shape.B} {shape.screen} mid={shape.mid} tile={tile}: " + ", ".join(f"{k} {lo} .. {hi}" for k, (lo, hi) in br.items()))
            for name, (lo, hi) in br.items():
                assert lo >= 200, (shape, tile, name, lo)
                assert hi - lo <= 0.02 * hi, (shape, tile, name, lo, hi)
    # a query that is masked out counts nothing at any screen — but the row with an inf, which the f32-row form keeps for every query
    for screen, reader in {(s.screen, sr.mid_reader(sr.form_of(s)) if mid == "on" else None)
                           for s in sr.SHAPES if (s.D, s.segs, s.mid) == (D, segs, mid) and sr.tiles_of(s) > 1}:
        lo, hi = case.per_query(screen, reader, 0)
        for name, v in hi.items():
            np.testing.assert_array_equal(v, np.full(256, 1 if (screen, name) == ("f32", "coarse") else 0))


def test_in_range_rows_pass_every_screen(oracle):
    """the models themselves (no slack) lose no in-range row of a case"""
    case = sr.Case.get(oracle, 384, "cosine")
    rows, qs = case.parts[0], case.qs
    tau = case.tau(case.bounds(256))
    inr = case.in_range(256)
    for keep in (sr.keep_int8(rows, qs, tau), sr.keep_bf16(rows, qs, tau), sr.keep_mid(rows, qs, tau), sr.keep_fine(rows, qs, tau)):
        for q in range(256):
            assert keep[case.opos[q, : inr[q]], q].all()


# ---- forms ----------------------------------------------------------------------------------------------------------------------------
def required_forms():
    """every form of the table in DESIGN.md §4 (The screens as numbers)"""
    need = set()
    for nt in (1, 2):
        for ncht, nch in ((1, 1), (2, 2), (3, 3), (4, 4), (0, 5), (6, 6), (0, 7), (8, 8)):
            need.add(sr.Drain(nt, ncht, nch, 4, True))
        need.add(sr.Drain(nt, 2, 2, 4, False))            # plain loads
    need |= {sr.Drain(2, 3, 3, 3, True), sr.Drain(2, 6, 6, 3, True)}  # three chunk buffers
    need |= {sr.Four(1, 4, 4, True), sr.Four(2, 4, 3, True)}           # 1..4 queries; kFlagFourWave at 16 and 64
    need |= {sr.Four(4, 4, 4, True), sr.Four(4, 8, 4, True)}           # the 128-query tile, two per CU and eight waves on one
    for nch in (1, 2, 3):
        for nh in (2, 4):
            need |= {sr.Hold(nch, nh, True), sr.Hold(nch, nh, False)}
    for nt in (1, 2, 4):
        need |= {sr.Mfma(nt, nt == 4, True, 4, 8 if nt == 4 else 4, True), sr.Mfma(nt, nt == 4, True, 6, 8 if nt == 4 else 4, True)}
        need.add(sr.Mfma(nt, nt == 4, False, 3 if nt == 4 else 2, 8 if nt == 4 else 4, True))
    need |= {sr.Mfma(2, True, True, 4, 8, True), sr.Mfma(2, True, True, 6, 8, True)}  # 512-d: the wide form at NT = 2
    need |= {sr.Wave(1, True), sr.Wave(4, True)}
    return need


def test_shapes_reach_every_form():
    reached = {}
    for s in sr.SHAPES:
        reached.setdefault(sr.form_of(s), []).append(s)
    missing = required_forms() - set(reached)
    assert not missing, missing
    # B = 1 and 4 and the flagged 16 and 64 reach the four-wave form, D = 384 / B = 100 the 128-query tile under kFlagTile128
    assert {s.B for s in reached[sr.Four(1, 4, 4, True)]} >= {1, 4, 16} and 64 in {s.B for s in reached[sr.Four(2, 4, 3, True)]}
    assert any(s.D == 384 and s.flags & sr.FLAG_TILE128 for s in reached[sr.Four(4, 4, 4, True)])
    # both copies of the mid test are read, the drain wave's at 64 queries, at one and two trips of the 16-byte loop
    mids = {(sr.mid_reader(sr.form_of(s)), s.D) for s in sr.SHAPES if s.mid == "on"}
    assert mids >= {(r, D) for r in ("fine_survivors", "drain_survivors") for D in (100, 384, 768)}
    # several segments: the drain form and the four-half hold kernel
    segs = {type(sr.form_of(s)).__name__ + str(getattr(sr.form_of(s), "nh", "")) for s in sr.SHAPES if s.segs}
    assert segs == {"Drain", "Hold4"}
    # every shape is one pass
    for s in sr.SHAPES:
        Dp = (s.D + 63) // 64 * 64
        assert s.B <= (sr.mfma8_pass_queries(Dp) if s.screen == "int8" else 4 if s.screen == "wave" else sr.mfma_pass_queries(Dp))


def test_scan_form_follows_the_launchers():
    assert sr.scan_form(256, 200, 0, "int8") == sr.Hold(2, 4, True)
    assert sr.scan_form(64, 768, 3 << 24, "int8") == sr.Drain(2, 6, 6, 3, True)
    assert sr.scan_form(64, 640, 1, "int8") == sr.Drain(2, 0, 5, 4, False)
    assert sr.scan_form(64, 512, 4 << 24, "bf16") == sr.Mfma(2, True, True, 4, 8, True)
    assert sr.scan_form(64, 384, 0, "bf16") == sr.Mfma(2, False, True, 4, 4, True)
    assert sr.scan_form(128, 384, 0, "f32") == sr.Mfma(4, True, False, 3, 8, True)
    assert sr.scan_form(64, 384, 0, "int8", six_copy=True) == sr.Six(2, 3)
    assert sr.scan_form(64, 384, sr.TUNE_NO_SIX, "int8", six_copy=True) == sr.Drain(2, 3, 3, 4, True)
    assert sr.scan_form(65, 384, 0, "int8", six_copy=True) == sr.Hold(3, 2, True)
    assert sr.scan_form(4, 384, 0, "int8", six_copy=True) == sr.Four(1, 4, 4, True)
    assert sr.scan_form(128, 768, 0, "int8") == sr.Four(4, 8, 4, True) and sr.scan_form(128, 512, 0, "int8") == sr.Four(4, 4, 4, True)
    assert sr.mfma8_pass_queries(384) == 256 and sr.mfma8_pass_queries(448) == 128 and sr.mfma8_pass_queries(1024) == 128
    assert sr.mfma_pass_queries(384) == 128 and sr.mfma_pass_queries(1024) == 64
    assert sr.six_pass(64, 384, 0, 1) and not sr.six_pass(64, 384, 1, 1) and not sr.six_pass(64, 448, 0, 1) and not sr.six_pass(4, 128, 0, 1)
