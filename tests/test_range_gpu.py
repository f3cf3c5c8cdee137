"""GPU: range search (pcv_searcher_search_range), through the C ABI.  The reference of every check is oracle.topk over all rows,
cut by the test on the REPORTED f32 score (computed here as hits_to_outputs computes it); where the corpus is too big for that,
search_vectors of the same searcher, cut the same way.  Ids and f32 scores are compared for equality."""
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384
PCV_ERR_UNSUPPORTED = 3
PCV_MAX_RANGE_ROWS = 1 << 24
FORCE_SIX = 1 << 31
INF = np.float32(np.inf)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def reported(c, metric):
    """hits_to_outputs: (float)c for cosine, max(0, 1 - c / dim) in f64 then f32 for the dot metric"""
    c = np.asarray(c, dtype=np.float64)
    if metric == "dot":
        d = 1.0 - c / np.float64(D)
        return np.where(d > 0.0, d, 0.0).astype(np.float32)
    return c.astype(np.float32)


def in_range(score, bound, metric):
    return score <= np.float32(bound) if metric == "dot" else score >= np.float32(bound)


def cut(ids, scores, bound, metric):
    """the hits of a best-first list that pass the bound: a prefix of it"""
    ok = in_range(scores, bound, metric)
    n = int(ok.sum())
    assert ok[:n].all()
    return ids[:n], scores[:n]


class Ranking:
    """oracle.topk over all rows for a set of queries: the canonical order of every searchable row"""

    def __init__(self, oracle, queries, rows, ids, metric):
        self.metric = metric
        pos, sc, cnt = oracle.topk(queries, rows, rows.shape[0], metric=1 if metric == "dot" else 0)
        self.pos, self.cnt = pos, cnt
        self.ids = np.where(pos >= 0, ids[np.maximum(pos, 0)], -1)
        self.scores = reported(sc, metric)

    def expect(self, q, bound, allowed_pos=None):
        n = int(self.cnt[q])
        ids, scores = self.ids[q, :n], self.scores[q, :n]
        if allowed_pos is not None:
            keep = np.isin(self.pos[q, :n], allowed_pos)
            ids, scores = ids[keep], scores[keep]
        return cut(ids, scores, bound, self.metric)


def check(got, want_ids, want_scores, q, max_results):
    ids, scores, counts, more = got
    n = min(len(want_ids), max_results)
    assert int(counts[q]) == n, (q, int(counts[q]), n, len(want_ids))
    assert bool(more[q]) == (len(want_ids) > max_results), q
    np.testing.assert_array_equal(ids[q, :n], want_ids[:n])
    np.testing.assert_array_equal(bits(scores[q, :n]), bits(want_scores[:n]))
    assert (ids[q, n:] == -1).all() and np.isnan(scores[q, n:]).all()


# ---- 1. every screen form, both metrics ----------------------------------------------------------------------------------
N_ANCHOR = 6
LEVELS = (0.999, 0.99, 0.95, 0.9)


def planted_corpus(metric, seed=5):
    """~6000 rows: Gaussian rows plus, per anchor row, groups of 12 rows at cosine 0.999, 0.99, 0.95 and 0.9 of it; for the dot
    metric every row times an amplitude of its own in [0.5, 1.5)"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((5700, D)).astype(np.float32)
    anchors = base[:N_ANCHOR]
    groups = []
    for a in anchors:
        u = a / np.linalg.norm(a)
        for cos in LEVELS:
            noise = rng.standard_normal((12, D))
            noise -= np.outer(noise @ u, u)
            noise /= np.linalg.norm(noise, axis=1, keepdims=True)
            groups.append((np.linalg.norm(a) * (cos * u + np.sqrt(1 - cos * cos) * noise)).astype(np.float32))
    rows = np.concatenate([base] + groups)
    rows = rows[rng.permutation(rows.shape[0])]
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(rows.shape[0], 1))).astype(np.float32)
    ids = (rng.permutation(rows.shape[0]) * 7 + 1000).astype(np.int64)
    return np.ascontiguousarray(rows), ids, anchors


def build_three_segments(ctx, metric, rows, ids, form):
    """source 1 in two segments (a small first add, then more than its spare room), source 2 in one"""
    s = pa.Searcher(ctx, D, metric)
    kernel, copy, mid, tuning = form
    s.set_kernel(kernel)
    s.set_screening_copy(copy)
    s.set_mid_copy(mid)
    s.set_tuning(tuning)
    s.add_rows(1, rows[:400], ids[:400])
    s.finalize()
    s.add_rows(1, rows[400:3400], ids[400:3400])
    s.add_rows(2, rows[3400:], ids[3400:])
    s.finalize()
    assert s.num_segments >= 3 and s.num_rows == rows.shape[0]
    return s


FORMS = {
    "wave": ("wave", "off", "off", 0),
    "mfma_f32": ("mfma", "off", "off", 0),
    "mfma_bf16": ("mfma", "bf16", "off", 0),
    "mfma_int8": ("mfma", "int8", "off", 0),
    "auto_six": ("auto", "auto", "off", FORCE_SIX),  # (the 6-bit copy is AUTO's: built beside the int8 copy AUTO keeps)
    "int8_mid": ("mfma", "int8", "on", 0),
}


@pytest.fixture(scope="module")
def planted(oracle):
    out = {}
    for metric in ("cosine", "dot"):
        rows, ids, anchors = planted_corpus(metric)
        rng = np.random.default_rng(17)
        queries = rng.standard_normal((200, D)).astype(np.float32)
        # the first queries are the anchors with a little noise, the rest Gaussian
        for i in range(60):
            queries[i] = anchors[i % N_ANCHOR] + 0.02 * rng.standard_normal(D).astype(np.float32)
        if metric == "dot":
            queries = (queries * rng.uniform(0.5, 1.5, size=(200, 1))).astype(np.float32)
            menu = [0.0, 0.2, 0.5, 0.8, 0.97, 1.0, 1.02, INF, -INF, -0.25]
        else:
            menu = [0.9995, 0.995, 0.97, 0.93, 0.5, 0.12, 0.0, -INF, INF, -0.05]
        bounds = np.array([menu[i % len(menu)] for i in range(200)], dtype=np.float32)
        out[metric] = (rows, ids, queries, bounds, Ranking(oracle, queries, rows, ids, metric))
    return out


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("form", list(FORMS))
def test_screen_forms(ctx, planted, form, metric):
    rows, ids, queries, bounds, rank = planted[metric]
    s = build_three_segments(ctx, metric, rows, ids, FORMS[form])
    total = 0
    for B in (1, 3, 64, 70, 200):
        for sources, allowed in ((None, None), ([2], np.arange(3400, rows.shape[0]))):
            if sources is not None and B not in (3, 70):
                continue
            got = s.search_range(sources, bounds[:B], queries[:B], rows.shape[0])
            st = s.last_stats()
            assert st["overflow_reruns"] <= 1
            if form == "auto_six" and B == 64:
                assert st["screen_bits"] == 6
            for q in range(B):
                wi, ws = rank.expect(q, bounds[q], allowed)
                check(got, wi, ws, q, rows.shape[0])
                total += len(wi)
    assert total > 10000  # the bounds were not all empty
    # a small max_results cuts every list and says so
    got = s.search_range(None, bounds[:70], queries[:70], 5)
    for q in range(70):
        wi, ws = rank.expect(q, bounds[q])
        check(got, wi, ws, q, 5)
    empty = s.search_range([], bounds[:3], queries[:3], 5)  # an empty filter matches nothing
    assert (empty[2] == 0).all() and not empty[3].any() and (empty[0] == -1).all()
    s.close()


# ---- 2. the edge of the bound --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_edge_of_the_bound(ctx, oracle, metric):
    rng = np.random.default_rng(23)
    rows = rng.standard_normal((3000, D)).astype(np.float32)
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(3000, 1))).astype(np.float32)
    rows[100:110] = rows[2000]  # ten exact copies of one row (eleven rows with one score), positions 100..109 and 2000
    rows[300:305] = 3.0 * rows[2500] / np.float32(np.linalg.norm(rows[2500]) / np.sqrt(D))  # dot: distance clamps to 0 for a like query
    ids = np.arange(3000, dtype=np.int64) + 50
    s = pa.Searcher(ctx, D, metric)
    s.add_rows(1, rows, ids)
    s.finalize()
    q = (rows[2000] + 0.3 * rng.standard_normal(D)).astype(np.float32)[None, :]
    rank = Ranking(oracle, q, rows, ids, metric)
    top_ids, top_sc, top_cnt = s.search_vectors(None, 40, q)
    np.testing.assert_array_equal(top_ids[0], rank.ids[0, :40])
    np.testing.assert_array_equal(bits(top_sc[0]), bits(rank.scores[0, :40]))
    stricter = INF if metric == "cosine" else -INF
    for j in (0, 5, 11, 12, 25, 39):
        sj = top_sc[0, j]
        wi, ws = rank.expect(0, sj)
        assert ids_of(wi).count(int(top_ids[0, j])) == 1  # bound = s returns the row
        check(s.search_range(None, sj, q, 3000), wi, ws, 0, 3000)
        tight = np.nextafter(sj, stricter)
        wi2, ws2 = rank.expect(0, tight)
        assert int(top_ids[0, j]) not in ids_of(wi2)  # the next f32 towards "stricter" does not
        check(s.search_range(None, tight, q, 3000), wi2, ws2, 0, 3000)
    # the eleven equal rows straddle the bound together and come in position order
    where = [k for k in range(40) if int(top_ids[0, k]) in set(range(150, 160)) | {2050}]
    assert len(where) == 11 and where == list(range(where[0], where[0] + 11))
    np.testing.assert_array_equal(top_ids[0, where], list(range(150, 160)) + [2050])
    sc = top_sc[0, where[0]]
    got = s.search_range(None, sc, q, 3000)
    assert int(got[2][0]) == where[0] + 11
    got = s.search_range(None, np.nextafter(sc, stricter), q, 3000)
    assert int(got[2][0]) == where[0]
    if metric == "dot":
        # the best rows all clamp to distance 0: bound 0 returns exactly those, ordered by c then position
        q0 = rows[300:301].copy()
        rank0 = Ranking(oracle, q0, rows, ids, metric)
        wi, ws = rank0.expect(0, 0.0)
        assert len(wi) >= 5 and (ws == 0).all()
        check(s.search_range(None, 0.0, q0, 3000), wi, ws, 0, 3000)
        assert int(s.search_range(None, -1e-30, q0, 10)[2][0]) == 0  # a negative bound matches nothing
    s.close()


def ids_of(a):
    return [int(x) for x in a]


# ---- 3. long lists -------------------------------------------------------------------------------------------------------
def test_long_lists(ctx):
    N, M = 300_000, 20_000
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, N, 0xA11CE)
    s.finalize()
    rows, _ = s.get_rows(np.array([12345, 777], dtype=np.int64))
    q = rows.astype(np.float32)
    before = s.search_vectors(None, 10, q)
    full = s.search_vectors(None, M + 500, q)
    plain_launches = s.last_stats()["scan_launches"]
    assert plain_launches >= (M + 500 + 127) // 128
    bounds = np.array([full[1][0, M - 1], full[1][1, M // 2]], dtype=np.float32)
    want = [cut(full[0][b], full[1][b], bounds[b], "cosine") for b in range(2)]
    assert len(want[0][0]) >= M and len(want[0][0]) < M + 500  # more than one LDS run, more than the default 8192 candidates
    got = s.search_range(None, bounds, q, M + 1000)
    st = s.last_stats()
    assert st["overflow_reruns"] <= 1 and st["scan_launches"] <= 2
    for b in range(2):
        check(got, want[b][0], want[b][1], b, M + 1000)
    assert not got[3].any()
    for m in (1000, 1):
        got = s.search_range(None, bounds, q, m)
        assert s.last_stats()["overflow_reruns"] <= 1 and s.last_stats()["scan_launches"] <= 2
        for b in range(2):
            check(got, want[b][0], want[b][1], b, m)
        assert got[3].all()
    # the scan state was left clean and no threshold leaked: a plain search returns what it did before
    after = s.search_vectors(None, 10, q)
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(bits(after[1]), bits(before[1]))
    s.close()


# ---- 4. hidden, updated and removed items, views, search by example ---------------------------------------------------------
def test_changes_views_and_like(ctx, oracle):
    metric = "cosine"
    rows, ids, anchors = planted_corpus(metric, seed=9)
    rng = np.random.default_rng(3)
    queries = np.concatenate([anchors[:4], rng.standard_normal((4, D)).astype(np.float32)])
    bounds = np.array([0.94, 0.985, 0.05, 0.1, 0.08, 0.12, -INF, 0.1], dtype=np.float32)
    N = rows.shape[0]
    s = build_three_segments(ctx, metric, rows, ids, ("auto", "auto", "auto", 0))

    def same_as_fresh(cur_rows, cur_ids, allowed=None, searcher=None):
        rank = Ranking(oracle, queries, cur_rows, cur_ids, metric)
        got = (searcher or s).search_range(None, bounds, queries, N)
        for q in range(len(queries)):
            wi, ws = rank.expect(q, bounds[q], allowed)
            check(got, wi, ws, q, N)
        return got

    base = same_as_fresh(rows, ids)
    # hidden rows are never in range and come back
    hide = np.unique(np.concatenate([base[0][0, :5], base[0][2, :50], base[0][6, 100:200]]))
    s.hide_items(hide)
    shown = ~np.isin(ids, hide)
    got = same_as_fresh(rows, ids, allowed=np.nonzero(shown)[0])
    assert not np.isin(got[0], hide).any()
    s.unhide_items(hide)
    again = same_as_fresh(rows, ids)
    np.testing.assert_array_equal(again[0], base[0])
    # updated items: as a searcher built from the new rows
    upd = ids[[10, 500, 3500, 5000]]
    new_rows = rows.copy()
    new_rows[[10, 500, 3500, 5000]] = (anchors[0] + 0.01 * rng.standard_normal((4, D))).astype(np.float32)
    s.update_items(upd, new_rows[[10, 500, 3500, 5000]])
    got = same_as_fresh(new_rows, ids)
    assert np.isin(upd, got[0][0, : int(got[2][0])]).all()
    # a view: only its rows
    allow = ids[::3]
    v = s.view(allow)
    same_as_fresh(new_rows, ids, allowed=np.arange(0, N, 3), searcher=v)
    v.close()
    # search by example: the planted copies of the item, itself first
    item = int(base[0][1, 0])
    items = s.search_range_like_item(None, 0.985, item, N)
    row_of = int(np.nonzero(ids == item)[0][0])
    rank1 = Ranking(oracle, new_rows[row_of : row_of + 1], new_rows, ids, metric)
    wi, ws = rank1.expect(0, 0.985)
    assert items[0].id == item and [it.id for it in items] == ids_of(wi) and len(items) >= 12
    np.testing.assert_array_equal(bits([it.score for it in items]), bits(ws))
    with pytest.raises(KeyError):
        s.search_range_like_item(None, 0.9, -12345, 10)
    # removed items: as a searcher built without them
    gone = ids[np.r_[5:40, 3390:3420, N - 7 : N]]
    s.remove_items(gone)
    stay = ~np.isin(ids, gone)
    same_as_fresh(new_rows[stay], ids[stay])
    s.close()


# ---- 5. the refusal --------------------------------------------------------------------------------------------------------
def test_refusal_beyond_max_range_rows(ctx):
    d, N = 64, PCV_MAX_RANGE_ROWS + 40_000
    s = pa.Searcher(ctx, d, "cosine")
    s.add_synthetic(1, N, 77)
    s.finalize()
    q = s.get_rows(np.array([5], dtype=np.int64))[0].astype(np.float32)
    before = s.search_vectors(None, 10, q)
    with pytest.raises(pa.PcvError) as e:
        s.search_range(None, -INF, q, 100)
    assert e.value.status == PCV_ERR_UNSUPPORTED
    msg = str(e.value)
    assert "search_range" in msg and "query 0" in msg and str(N) in msg and "PCV_MAX_RANGE_ROWS" in msg
    after = s.search_vectors(None, 10, q)  # the searcher stays usable
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(bits(after[1]), bits(before[1]))
    got = s.search_range(None, 0.5, q, 100)  # ... and so does range search with a bound that lists fewer rows
    assert int(got[2][0]) >= 1 and got[0][0, 0] == 5
    s.close()


# ---- 6. full size, modest --------------------------------------------------------------------------------------------------
def test_full_size_auto(ctx):
    N, B, K = 10_000_000, 16, 2048
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, N, 0xBEEF)
    s.finalize()
    rng = np.random.default_rng(41)
    pick = rng.integers(0, N, size=B)
    rows, _ = s.get_rows(pick.astype(np.int64))
    q = (rows + 0.05 * rng.standard_normal((B, D))).astype(np.float32)
    full = s.search_vectors(None, K, q)
    assert (full[2] == K).all()
    # bounds from the top-k itself: between 0 and ~2000 matches per query
    at = [0, 1, 3, 10, 50, 100, 127, 128, 129, 300, 700, 1000, 1500, 1900, 2000, 2040]
    bounds = np.array([full[1][b, at[b]] for b in range(B)], dtype=np.float32)
    bounds[0] = np.nextafter(full[1][0, 0], INF)  # nothing
    got = s.search_range(None, bounds, q, K)
    st = s.last_stats()
    assert st["scan_launches"] <= 2 and st["overflow_reruns"] <= 1
    for b in range(B):
        wi, ws = cut(full[0][b], full[1][b], bounds[b], "cosine")
        assert len(wi) < K  # the cut is inside the list, so the list is a complete reference
        check(got, wi, ws, b, K)
    assert int(got[2][0]) == 0
    s.close()


def test_cpp_mirror_range_program():
    src = os.path.join(ROOT, "tests", "cpp", "range_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "range_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "range_mirror_test: ok" in r.stdout


def test_unfinalized_searcher_gives_the_error_of_search(ctx):
    """Rows added without finalize: search_range refuses as search does — same status, same text but for the call's name — and
    works once the searcher is finalized."""
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((40, 32)).astype(np.float32)
    s = pa.Searcher(ctx, 32, "cosine")
    s.add_rows(1, rows, np.arange(40))
    with pytest.raises(pa.PcvError) as plain:
        s.search_vectors(None, 5, rows[:1])
    with pytest.raises(pa.PcvError) as ranged:
        s.search_range(None, 0.5, rows[:1], 5)
    assert ranged.value.status == plain.value.status
    tail = "rows were added or cleared without pcv_searcher_finalize"
    assert str(plain.value).endswith(tail) and str(ranged.value).endswith("search_range: " + tail)
    s.finalize()
    ids, _scores, counts, more = s.search_range(None, 0.5, rows[:1], 5)
    assert counts[0] == 1 and ids[0, 0] == 0 and not more[0]
    s.close()
