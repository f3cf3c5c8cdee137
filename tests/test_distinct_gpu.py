"""GPU: distinct results (pcv_searcher_search_distinct), through the C ABI.  The reference of every check is built per query in two
steps: oracle.topk over all rows gives the ranked list L, and the greedy walk below runs over L with orc_canonical_score(row, kept
row, metric 0) >= (double)threshold as the duplicate test.  Kept ids, f32 score bits, counts, similar, examined and more are
compared for equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384
FORCE_SIX = 1 << 31
_FP = C.POINTER(C.c_float)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def reported(c, metric, dim):
    """hits_to_outputs: (float)c for cosine, max(0, 1 - c / dim) in f64 then f32 for the dot metric"""
    c = np.asarray(c, dtype=np.float64)
    if metric == "dot":
        d = 1.0 - c / np.float64(dim)
        return np.where(d > 0.0, d, 0.0).astype(np.float32)
    return c.astype(np.float32)


def default_pool(k):
    return min(4096, max(128, 8 * k))


class Reference:
    """The ranked list of every query (oracle.topk over all rows) and the greedy walk over it.  Pair cosines are
    orc_canonical_score(row, kept row, D, 0), computed when the walk asks and remembered: the walks of one corpus share them."""

    def __init__(self, oracle, queries, rows, ids, metric, depth=None):
        self.lib = oracle.lib
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.ids, self.metric, self.dim = ids, metric, self.rows.shape[1]
        n = self.rows.shape[0]
        self.pos, self.sc, self.cnt = oracle.topk(queries, self.rows, depth or n, metric=1 if metric == "dot" else 0)
        self.ptr = [C.cast(self.rows.ctypes.data + i * self.dim * 4, _FP) for i in range(n)]
        self.pairs = {}
        self.walks = {}

    def cos(self, a, b):
        c = self.pairs.get((a, b))
        if c is None:
            c = self.pairs[(a, b)] = self.lib.orc_canonical_score(self.ptr[a], self.ptr[b], self.dim, 0)
        return c

    def walk(self, q, k, threshold, pool, allowed=None):
        """-> (kept ids, their f32 scores, similar, examined, more)"""
        key = (q, k, float(np.float32(threshold)), pool, None if allowed is None else allowed.tobytes())
        if key in self.walks:
            return self.walks[key]
        n = int(self.cnt[q])
        L, sc = self.pos[q, :n], self.sc[q, :n]
        if allowed is not None:
            ok = np.isin(L, allowed)
            L, sc = L[ok], sc[ok]
        thr = float(np.float32(threshold))  # (double)threshold
        kept, kept_sc, similar, examined = [], [], [], 0
        for row, s in zip(L[:pool].tolist(), sc[:pool].tolist()):
            examined += 1
            dup = next((j for j, kr in enumerate(kept) if self.cos(row, kr) >= thr), None)  # (NaN: not a duplicate)
            if dup is None:
                kept.append(row)
                kept_sc.append(s)
                similar.append(0)
                if len(kept) == k:
                    break
            else:
                similar[dup] += 1
        more = len(kept) < k and examined == pool and len(L) > pool
        out = (self.ids[kept] if kept else np.zeros(0, np.int64), reported(kept_sc, self.metric, self.dim), similar, examined, more)
        self.walks[key] = out
        return out


def check(got, want, q, k):
    ids, scores, counts, similar, examined, more = got
    w_ids, w_scores, w_similar, w_examined, w_more = want
    n = len(w_ids)
    print("query %d: kept %d/%d examined %d/%d more %s/%s" % (q, int(counts[q]), n, int(examined[q]), w_examined, bool(more[q]), w_more))
    assert int(counts[q]) == n, (q, int(counts[q]), n)
    np.testing.assert_array_equal(ids[q, :n], w_ids)
    np.testing.assert_array_equal(bits(scores[q, :n]), bits(w_scores))
    np.testing.assert_array_equal(similar[q, :n], np.array(w_similar, dtype=np.int32))
    assert int(examined[q]) == w_examined, (q, int(examined[q]), w_examined)
    assert bool(more[q]) == w_more, q
    assert (ids[q, n:] == -1).all() and np.isnan(scores[q, n:]).all() and (similar[q, n:] == 0).all()
    assert ids.shape == (len(counts), k)


# ---- 1. planted families, every screen form, both metrics -------------------------------------------------------------------
N_ANCHOR = 8
FAMILIES = ((0.999, 20), (0.99, 20), (0.97, 20), (0.9, 12))


def planted_corpus(metric, dim=D, seed=5, n_base=2600, families=FAMILIES, n_anchor=N_ANCHOR):
    """Gaussian rows plus, per anchor row, families at a given cosine of it (the construction of test_range_gpu.py); rows shuffled,
    ids permuted and not contiguous; for the dot metric every row times an amplitude of its own in [0.5, 1.5)"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n_base, dim)).astype(np.float32)
    anchors = base[:n_anchor].copy()
    groups = []
    for a in anchors:
        u = a / np.linalg.norm(a)
        for cos, size in families:
            noise = rng.standard_normal((size, dim))
            noise -= np.outer(noise @ u, u)
            noise /= np.linalg.norm(noise, axis=1, keepdims=True)
            groups.append((np.linalg.norm(a) * (cos * u + np.sqrt(1 - cos * cos) * noise)).astype(np.float32))
    rows = np.concatenate([base] + groups)
    rows = rows[rng.permutation(rows.shape[0])]
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(rows.shape[0], 1))).astype(np.float32)
    ids = (rng.permutation(rows.shape[0]) * 7 + 1000).astype(np.int64)
    return np.ascontiguousarray(rows), ids, anchors


def planted_queries(metric, anchors, dim, seed=17):
    """8 noisy anchors, then 8 Gaussian rows"""
    rng = np.random.default_rng(seed)
    queries = rng.standard_normal((16, dim)).astype(np.float32)
    for i in range(8):
        queries[i] = anchors[i % len(anchors)] + 0.02 * rng.standard_normal(dim).astype(np.float32)
    if metric == "dot":
        queries = (queries * rng.uniform(0.5, 1.5, size=(16, 1))).astype(np.float32)
    return queries


SPLIT = (400, 2000)  # source 1: rows [0, 400) and [400, 2000) in two segments; source 2: the rest


def build_three_segments(ctx, metric, rows, ids, form, dim=D):
    s = pa.Searcher(ctx, dim, metric)
    kernel, copy, mid, tuning = form
    s.set_kernel(kernel)
    s.set_screening_copy(copy)
    s.set_mid_copy(mid)
    s.set_tuning(tuning)
    a, b = SPLIT
    s.add_rows(1, rows[:a], ids[:a])
    s.finalize()
    s.add_rows(1, rows[a:b], ids[a:b])
    s.add_rows(2, rows[b:], ids[b:])
    s.finalize()
    assert s.num_segments >= 3 and s.num_rows == rows.shape[0]
    return s


FORMS = {  # the table of test_range_gpu.py
    "wave": ("wave", "off", "off", 0),
    "mfma_f32": ("mfma", "off", "off", 0),
    "mfma_bf16": ("mfma", "bf16", "off", 0),
    "mfma_int8": ("mfma", "int8", "off", 0),
    "auto_six": ("auto", "auto", "off", FORCE_SIX),
    "int8_mid": ("mfma", "int8", "on", 0),
}
THRESHOLDS = (0.985, 0.95, 0.5, 1.0)


@pytest.fixture(scope="module")
def planted(oracle):
    out = {}
    for metric, dim in (("cosine", D), ("dot", D), ("cosine", 100)):
        rows, ids, anchors = planted_corpus(metric, dim)
        queries = planted_queries(metric, anchors, dim)
        out[(metric, dim)] = (rows, ids, queries, Reference(oracle, queries, rows, ids, metric))
    return out


def run_planted(ctx, planted, form, metric, dim):
    rows, ids, queries, ref = planted[(metric, dim)]
    s = build_three_segments(ctx, metric, rows, ids, FORMS[form], dim)
    collapsed = 0
    for B in (1, 3, 16):
        for k in (1, 10, 128):
            for thr in THRESHOLDS:
                got = s.search_distinct(None, k, queries[:B], thr)
                for q in range(B):
                    want = ref.walk(q, k, thr, default_pool(k))
                    check(got, want, q, k)
                    collapsed += sum(want[2])
    assert collapsed > 1000  # the families were met
    # a source filter: only the rows of source 2
    allowed = np.arange(SPLIT[1], rows.shape[0])
    got = s.search_distinct([2], 10, queries[:16], 0.95, pool=200)
    for q in range(16):
        check(got, ref.walk(q, 10, 0.95, 200, allowed), q, 10)
    empty = s.search_distinct([], 10, queries[:3], 0.95)  # an empty filter matches nothing
    assert (empty[2] == 0).all() and (empty[0] == -1).all() and (empty[4] == 0).all() and not empty[5].any()
    s.close()
    return ref


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("form", list(FORMS))
def test_planted_families(ctx, planted, form, metric):
    ref = run_planted(ctx, planted, form, metric, D)
    if metric == "cosine":
        # an anchor query meets the anchor, then its 0.999, 0.99 and 0.97 families — duplicates of the anchor at 0.95, though the
        # members of the 0.97 family are none of each other (about 0.941) —, then the 0.9 family, whose members are kept one by one
        for q in range(8):
            assert (len(ref.walk(q, 10, 0.95, 128)[0]), ref.walk(q, 10, 0.95, 128)[3]) == (10, 70)
            assert (len(ref.walk(q, 10, 0.985, 128)[0]), ref.walk(q, 10, 0.985, 128)[3]) == (10, 50)


def test_planted_families_padded_width(ctx, planted):
    """D = 100: padded rows, no multiple of 128 or of 16"""
    run_planted(ctx, planted, "mfma_int8", "cosine", 100)


@pytest.mark.parametrize("dim", [768, 2048])
def test_wide_rows_take_smaller_tiles(ctx, oracle, dim):
    """Rows too wide for two LDS tiles of 32: the select step works with 16 (768-d) and 8 (2048-d) rows a tile"""
    rows, ids, anchors = planted_corpus("cosine", dim, seed=12, n_base=500, families=((0.999, 9), (0.97, 9), (0.9, 5)), n_anchor=3)
    queries = planted_queries("cosine", anchors, dim)[:4]
    ref = Reference(oracle, queries, rows, ids, "cosine")
    s = pa.Searcher(ctx, dim, "cosine")
    s.add_rows(1, rows, ids)
    s.finalize()
    for k, thr, pool in ((10, 0.95, 128), (40, 0.985, 200), (128, 0.5, 300)):
        got = s.search_distinct(None, k, queries, thr, pool=pool)
        for q in range(4):
            check(got, ref.walk(q, k, thr, pool), q, k)
    assert sum(ref.walk(0, 10, 0.95, 128)[2]) >= 18
    s.close()


# ---- 2. more than one pass, and the pool limit -----------------------------------------------------------------------------
def test_passes_and_pool_limit(ctx, oracle):
    rows, ids, anchors = planted_corpus("cosine", D, seed=21, families=((0.999, 300),), n_anchor=2)
    rng = np.random.default_rng(4)
    queries = np.concatenate([anchors + 0.02 * rng.standard_normal((2, D)).astype(np.float32), rng.standard_normal((3, D)).astype(np.float32)])
    ref = Reference(oracle, queries, rows, ids, "cosine")
    s = build_three_segments(ctx, "cosine", rows, ids, ("auto", "auto", "auto", 0))
    before = s.search_vectors(None, 10, queries)
    wide = s.search_distinct(None, 5, queries, 0.95, pool=1024)
    st = s.last_stats()
    for q in range(5):
        check(wide, ref.walk(q, 5, 0.95, 1024), q, 5)
    assert (wide[4][:2] > 256).all() and (wide[2] == 5).all()  # at least three passes for the family queries
    assert 3 <= st["scan_launches"] <= (1024 + 127) // 128 + 1
    assert not wide[5].any()
    narrow = s.search_distinct(None, 5, queries, 0.95, pool=128)
    for q in range(5):
        check(narrow, ref.walk(q, 5, 0.95, 128), q, 5)
    assert (narrow[2][:2] < 5).all() and narrow[5][:2].all() and (narrow[4][:2] == 128).all()
    # a query that finished in the first pass carries the same outputs in both calls
    for q in (2, 3, 4):
        assert int(wide[4][q]) <= 128 and not narrow[5][q]
        for a, b in zip(wide, narrow):
            np.testing.assert_array_equal(np.atleast_1d(a[q]).view(np.uint8), np.atleast_1d(b[q]).view(np.uint8))
    after = s.search_vectors(None, 10, queries)  # the scan state was left clean
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(bits(after[1]), bits(before[1]))
    s.close()


# ---- 3. the edge of the threshold -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_edge_of_the_threshold(ctx, oracle, metric):
    rng = np.random.default_rng(23)
    N = 600
    rows = rng.standard_normal((N, D)).astype(np.float32)
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(N, 1))).astype(np.float32)
    rows[20] = (1.3 * rows[10] + 0.25 * rng.standard_normal(D)).astype(np.float32)  # a pair at cosine about 0.97, norms unequal
    rows[100:109] = rows[500]  # ten equal rows: positions 100..108 and 500
    ids = np.arange(N, dtype=np.int64) * 3 + 50
    s = pa.Searcher(ctx, D, metric)
    s.add_rows(1, rows, ids)
    s.finalize()
    q = np.stack([rows[10] + 0.01 * rng.standard_normal(D), rows[500]]).astype(np.float32)
    ref = Reference(oracle, q, rows, ids, metric)
    assert set(ref.pos[0, :2].tolist()) == {10, 20}
    first, second = ref.pos[0, :2].tolist()
    c = ref.cos(second, first)
    lo = np.float32(c)
    if float(lo) > c:
        lo = np.nextafter(lo, np.float32(-np.inf))
    hi = np.nextafter(lo, np.float32(np.inf))
    assert float(lo) <= c < float(hi)
    for thr, collapses in ((lo, True), (hi, False)):
        got = s.search_distinct(None, 10, q[:1], thr)
        check(got, ref.walk(0, 10, thr, 128), 0, 10)
        assert int(got[3][0, 0]) == (1 if collapses else 0)
        assert (int(got[0][0, 1]) == int(ids[second])) == (not collapses)
    # ten exact copies are one hit at threshold 1.0 (for this row the canonical cosine with itself is not below 1: the quotient
    # dot / (sqrt(n) sqrt(n)) rounds to 1 or the double above it; rows where it rounds below 1 are no duplicates at 1.0, by definition)
    assert ref.cos(100, 500) >= 1.0
    got = s.search_distinct(None, 10, q, 1.0)
    check(got, ref.walk(1, 10, 1.0, 128), 1, 10)
    assert int(got[0][1, 0]) == int(ids[100]) and int(got[3][1, 0]) == 9
    assert not np.isin(ids[[101, 108, 500]], got[0][1]).any()
    s.close()


def test_rows_without_a_cosine_and_the_end_of_the_list(ctx, oracle):
    """A zero row under the dot metric is searchable, is no duplicate of anything and absorbs nothing; a list that ends exactly at
    `pool` has no more rows"""
    rng = np.random.default_rng(29)
    N = 100
    rows = rng.standard_normal((N, D)).astype(np.float32)
    rows[[7, 60]] = 0.0
    rows[30:36] = rows[5] * np.linspace(0.5, 3.0, 6, dtype=np.float32)[:, None]  # one direction, six norms
    ids = np.arange(N, dtype=np.int64) + 9
    s = pa.Searcher(ctx, D, "dot")
    s.add_rows(1, rows, ids)
    s.finalize()
    q = rng.standard_normal((3, D)).astype(np.float32)
    ref = Reference(oracle, q, rows, ids, "dot")
    for thr in (0.5, -0.5, 1.0):
        got = s.search_distinct(None, 128, q, thr, pool=128)
        for b in range(3):
            want = ref.walk(b, 128, thr, 128)
            check(got, want, b, 128)
            assert want[3] == N and not want[4]
            where = [int(np.nonzero(got[0][b] == i)[0][0]) for i in ids[[7, 60]]]  # both zero rows are kept ...
            assert all(int(got[3][b, w]) == 0 for w in where)                      # ... and nothing was dropped for them
    assert sum(ref.walk(0, 128, 0.5, 128)[2]) >= 5  # the six rows of one direction are one hit
    # pool == the number of rows: nothing more; one row fewer in the pool: more
    copies = np.repeat(rows[5:6], 129, axis=0)
    for n, more in ((128, False), (129, True)):
        t = pa.Searcher(ctx, D, "cosine")
        t.add_rows(1, copies[:n], np.arange(n, dtype=np.int64))
        t.finalize()
        got = t.search_distinct(None, 5, rows[5:6], 1.0, pool=128)
        assert int(got[2][0]) == 1 and int(got[0][0, 0]) == 0 and int(got[3][0, 0]) == 127 and int(got[4][0]) == 128
        assert bool(got[5][0]) == more
        t.close()
    s.close()


# ---- 4. hidden, updated and removed items, a view, search by example -------------------------------------------------------
def test_changes_views_and_like(ctx, oracle):
    metric = "cosine"
    rows, ids, anchors = planted_corpus(metric, seed=9)
    rng = np.random.default_rng(3)
    queries = np.concatenate([anchors[:4], rng.standard_normal((4, D)).astype(np.float32)])
    N = rows.shape[0]
    K, THR, POOL = 10, 0.95, 256
    s = build_three_segments(ctx, metric, rows, ids, ("auto", "auto", "auto", 0))

    def same_as_fresh(cur_rows, cur_ids, allowed=None, searcher=None):
        ref = Reference(oracle, queries, cur_rows, cur_ids, metric, depth=600)
        got = (searcher or s).search_distinct(None, K, queries, THR, pool=POOL)
        for q in range(len(queries)):
            check(got, ref.walk(q, K, THR, POOL, allowed), q, K)
        return got

    base = same_as_fresh(rows, ids)
    assert (base[3][:4, 0] >= 60).all()  # the anchors stand for their families
    # hidden rows are not walked and come back
    hide = np.unique(np.concatenate([base[0][0, :3], base[0][5, :6]]))
    s.hide_items(hide)
    got = same_as_fresh(rows, ids, allowed=np.nonzero(~np.isin(ids, hide))[0])
    assert not np.isin(got[0], hide).any()
    s.unhide_items(hide)
    again = same_as_fresh(rows, ids)
    np.testing.assert_array_equal(again[0], base[0])
    # updated items: as a searcher built from the new rows
    at = [10, 500, 2500, 3000]
    new_rows = rows.copy()
    new_rows[at] = (anchors[0] + 0.01 * rng.standard_normal((4, D))).astype(np.float32)
    s.update_items(ids[at], new_rows[at])
    same_as_fresh(new_rows, ids)
    # a view: only its rows
    v = s.view(ids[::3])
    same_as_fresh(new_rows, ids, allowed=np.arange(0, N, 3), searcher=v)
    v.close()
    # search by example: the item itself first, then distinct neighbours
    item = int(base[0][1, 0])
    row_of = int(np.nonzero(ids == item)[0][0])
    items = s.search_distinct_like_item(None, K, item, THR, pool=POOL)
    ref1 = Reference(oracle, new_rows[row_of : row_of + 1], new_rows, ids, metric, depth=600)
    w_ids, w_scores, _sim, _ex, _more = ref1.walk(0, K, THR, POOL)
    assert items[0].id == item and [it.id for it in items] == [int(x) for x in w_ids] and len(items) == K
    np.testing.assert_array_equal(bits([it.score for it in items]), bits(w_scores))
    with pytest.raises(KeyError):
        s.search_distinct_like_item(None, K, -12345, THR)
    # removed items: as a searcher built without them
    gone = ids[np.r_[5:40, 1990:2020, N - 7 : N]]
    s.remove_items(gone)
    stay = ~np.isin(ids, gone)
    same_as_fresh(new_rows[stay], ids[stay])
    s.close()


# ---- 5. the refusals ---------------------------------------------------------------------------------------------------------
def test_unfinalized_searcher_gives_the_error_of_search(ctx):
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((40, 32)).astype(np.float32)
    s = pa.Searcher(ctx, 32, "cosine")
    s.add_rows(1, rows, np.arange(40))
    with pytest.raises(pa.PcvError) as plain:
        s.search_vectors(None, 5, rows[:1])
    with pytest.raises(pa.PcvError) as distinct:
        s.search_distinct(None, 5, rows[:1], 0.9)
    assert distinct.value.status == plain.value.status
    tail = "rows were added or cleared without pcv_searcher_finalize"
    assert str(plain.value).endswith(tail) and str(distinct.value).endswith("search_distinct: " + tail)
    s.finalize()
    ids, _scores, counts, similar, examined, more = s.search_distinct(None, 5, rows[:1], 0.9)
    assert counts[0] == 5 and ids[0, 0] == 0 and examined[0] == 5 and not more[0] and not similar.any()
    s.close()


# ---- 6. the C++ mirror -------------------------------------------------------------------------------------------------------
def test_cpp_mirror_distinct_program():
    src = os.path.join(ROOT, "tests", "cpp", "distinct_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "distinct_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "distinct_mirror_test: ok" in r.stdout
