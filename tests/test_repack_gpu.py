"""GPU: a repacked copy is the copy a fresh build makes.  Searcher A is built from the final rows; searcher B starts with other
values in ~200 rows, takes the final values through update_items, and has ~200 ids of the same blocks hidden and unhidden.  Both
must then return the same hits, bit for bit, and let the same number of rows through the coarse and mid screens of a range pass
(whose thresholds are fixed before the scan: RangeRec in csrc/scan.h) — the counts move as soon as one repacked row scale, block
scale or code differs from the built one."""
import numpy as np
import pytest

import perceive_amd as pa

pytestmark = pytest.mark.gpu

N, N_FIRST = 3000, 1500  # 93 full blocks and one of 24 rows; the second add_rows finishes block 46 (rows 1472..1503)
ZERO_ROW, INF_ROW, DOMINANT_ROW = 77, 1490, 2050
FORCE_SIX = 0x80000000
_cases = {}


def reported(c, metric, D):
    """the f32 score a hit carries: (float)c for cosine, the distance max(0, 1 - c / dim) for the dot metric"""
    c = np.asarray(c, dtype=np.float64)
    if metric == "dot":
        d = 1.0 - c / np.float64(D)
        return np.where(d > 0.0, d, 0.0).astype(np.float32)
    return c.astype(np.float32)


def case(oracle, D, metric):
    """Rows, ids, queries, the rows searcher B starts with, and range bounds from the oracle — once per (D, metric)."""
    if (D, metric) in _cases:
        return _cases[D, metric]
    rng = np.random.default_rng(1000 + D)
    final = (rng.standard_normal((N, D)) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
    final[ZERO_ROW] = 0.0
    final[INF_ROW, 3] = np.inf
    final[DOMINANT_ROW] *= 0.01
    final[DOMINANT_ROW, 0] = 20.0  # one component far above the rest of its block
    ids = rng.permutation(10 * N)[:N].astype(np.int64)
    queries = rng.standard_normal((64, D)).astype(np.float32)
    # rows that differ in B at first: the dominant row, the non-finite row, the partial last block, both sides of the block
    # boundary the second add_rows call crosses, and others all over the segment
    changed = np.unique(np.concatenate([[DOMINANT_ROW, INF_ROW, 1503, 1504], np.arange(2976, N), rng.choice(N, 170, replace=False)]))
    changed = changed[changed != ZERO_ROW]
    start = final.copy()
    start[changed] = (rng.standard_normal((changed.size, D)) * rng.uniform(0.5, 2.0, (changed.size, 1))).astype(np.float32)
    # hidden and unhidden: rows of the updated blocks (updated ones among them), the all-zero row, and others
    blocks = np.unique(changed // 32)
    hidden = np.unique(np.concatenate([[ZERO_ROW, DOMINANT_ROW + 1], changed[::3], np.minimum(blocks[::2] * 32 + 5, N - 1),
                                       rng.choice(N, 100, replace=False)]))
    # bounds: the reported score of each query's 60th best row, so that 20..200 rows are in range
    _, sc, cnt = oracle.topk(queries, final, 200, metric=1 if metric == "dot" else 0)
    assert (cnt == 200).all()
    rep = reported(sc, metric, D)
    bounds = rep[:, 59].copy()
    in_range = (rep <= bounds[:, None]).sum(1) if metric == "dot" else (rep >= bounds[:, None]).sum(1)
    assert (in_range >= 20).all() and (in_range < 200).all()
    _cases[D, metric] = (final, ids, queries, changed, start, hidden, bounds, in_range)
    return _cases[D, metric]


def build(ctx, D, metric, screen, mid, tuning, rows, ids):
    s = pa.Searcher(ctx, D, metric)
    s.set_tuning(tuning)
    s.set_screening_copy(screen)
    s.set_mid_copy(mid)
    s.add_rows(1, rows[:N_FIRST], ids[:N_FIRST])
    s.finalize()
    s.add_rows(1, rows[N_FIRST:], ids[N_FIRST:])  # finishes block 46 of the finalized segment
    s.finalize()
    assert s.num_segments == 1 and s.num_rows == N
    return s


@pytest.mark.parametrize("screen,mid,tuning", [("int8", "off", 0), ("int8", "on", 0), ("bf16", "off", 0), ("bf16", "on", 0),
                                               ("auto", "off", FORCE_SIX)])  # AUTO (int8) builds the 6-bit copy beside it
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("D", [100, 384])  # 100: padded to 128 features, which the int8 copy pads on (its chunk is 128 wide)
def test_repacked_copies_are_the_built_ones(ctx, oracle, D, metric, screen, mid, tuning):
    final, ids, queries, changed, start, hidden, bounds, in_range = case(oracle, D, metric)
    a = build(ctx, D, metric, screen, mid, tuning, final, ids)
    b = build(ctx, D, metric, screen, mid, tuning, start, ids)
    found, n_changed = b.update_items(ids[changed], final[changed])
    assert found.all() and n_changed == changed.size
    assert b.hide_items(ids[hidden]) == hidden.size
    assert b.unhide_items(ids[hidden]) == hidden.size
    assert b.hidden_rows == 0
    for B in (4, 16, 64):
        for k in (10, 300):
            ids_a, sc_a, cnt_a = a.search_vectors(None, k, queries[:B])
            ids_b, sc_b, cnt_b = b.search_vectors(None, k, queries[:B])
            np.testing.assert_array_equal(ids_b, ids_a)
            np.testing.assert_array_equal(sc_b.view(np.uint32), sc_a.view(np.uint32))
            np.testing.assert_array_equal(cnt_b, cnt_a)
    # A's hits are the oracle's (which gives the all-zero row under cosine and the non-finite row no score, as the searcher does)
    ids_a, sc_a, cnt_a = a.search_vectors(None, 10, queries)
    opos, osc, ocnt = oracle.topk(queries, final, 10, metric=1 if metric == "dot" else 0)
    assert (ocnt == 10).all() and not np.isin(opos, [INF_ROW] + ([ZERO_ROW] if metric == "cosine" else [])).any()
    np.testing.assert_array_equal(ids_a, ids[opos])
    np.testing.assert_allclose(sc_a, reported(osc, metric, D), rtol=0, atol=1e-7)
    np.testing.assert_array_equal(cnt_a, ocnt)
    got_a = a.search_range(None, bounds, queries, 256)
    st_a = a.last_stats()
    got_b = b.search_range(None, bounds, queries, 256)
    st_b = b.last_stats()
    np.testing.assert_array_equal(got_a[2], in_range)
    np.testing.assert_array_equal(got_b[2], got_a[2])
    np.testing.assert_array_equal(got_b[3], got_a[3])
    for q in range(queries.shape[0]):
        n = int(got_a[2][q])
        np.testing.assert_array_equal(got_b[0][q, :n], got_a[0][q, :n])
        np.testing.assert_array_equal(got_b[1][q, :n].view(np.uint32), got_a[1][q, :n].view(np.uint32))
    print(f"survivors D={D} {metric} {screen} mid={mid} tuning={tuning:#x}: coarse {st_a['coarse_survivors']} / {st_b['coarse_survivors']}, "
          f"mid {st_a['mid_survivors']} / {st_b['mid_survivors']}, narrow {st_a['narrow_survivors']} / {st_b['narrow_survivors']}")
    # (only a pass that streams the int8 copy reads the mid copy: its bound needs |q'|_1 from the int8 query quantisation)
    assert st_a["mid_copy"] == st_b["mid_copy"] == (1 if mid == "on" and screen == "int8" else 0)
    assert st_b["coarse_survivors"] == st_a["coarse_survivors"]
    assert st_b["mid_survivors"] == st_a["mid_survivors"]
    a.close()
    b.close()
