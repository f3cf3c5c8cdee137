"""GPU: top-m labels (pcv_searcher_assign_top), through the Python mirror of the C ABI.  The reference of every check is
assign_top_ref.py: the oracle's canonical score of every (row, label) that can be listed, the m best by (c descending, label
ascending) within the bound; labels, f32 score bits, counts, ids and the rows per label are compared for equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from assign_top_ref import assign_top_reference, bits, canonical_norms, check_assign_top
from duplicates_ref import build, make_ids, neighbour
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384


def margin(dim):
    """selfjoin_margin at the padded dimension (selfjoin_kernels.hip)"""
    dp = (dim + 63) // 64 * 64
    return 0.00783 + 1.02 * ((dp + 16) * 1.2e-7) + 1e-6


def same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)


# ---- 1. golden corpora ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("name", ["scan_n77_d100", "scan_n1000_d384"])
def test_golden(ctx, oracle, golden_dir, name, metric):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    rows = np.array(g["corpus"], dtype=np.float32)
    rng = np.random.default_rng(21)
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(rows.shape[0], 1))).astype(np.float32)
    rows = np.ascontiguousarray(rows)
    n, dim = rows.shape
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids, metric)
    for K in (1, 5, 37):
        labels = rng.standard_normal((K, dim)).astype(np.float32)
        labels[K // 2] = rows[3]
        s_ids, s_scores, s_counts = s.search_vectors(None, n, labels)
        at = [{int(i): p for p, i in enumerate(s_ids[j, : s_counts[j]].tolist())} for j in range(K)]
        plain = s.assign(None, labels)
        for m in (1, 2, 3, 8):
            got = s.assign_top(None, labels, m)
            want = assign_top_reference(oracle, rows, labels, m, None, metric)
            check_assign_top(got, want, ids)
            st = s.last_assign_top_stats()
            assert st["rows"] == n and st["m"] == m and st["label_tiles"] == 1 and st["tile_labels"] == 128 and st["reruns"] == 0
            assert st["listed"] == got[3].sum() == want[2].sum() >= (n - 5) * min(m, K) and st["candidates"] >= st["listed"]
            assert got[0][3, 0] == K // 2 or metric == "dot"
            if m == 1:  # what assign gives, bit for bit
                np.testing.assert_array_equal(got[0][:, 0], plain[0])
                np.testing.assert_array_equal(bits(got[1][:, 0]), bits(plain[1]))
                np.testing.assert_array_equal(got[2], plain[2])
                np.testing.assert_array_equal(got[4], plain[3])
            # the scores are those of a search with the labels as queries, for the same pairs
            for r in range(0, n, 7):
                for slot in range(got[3][r]):
                    j = int(got[0][r, slot])
                    assert bits(got[1][r, slot : slot + 1])[0] == bits(s_scores[j, at[j][int(ids[r])] : at[j][int(ids[r])] + 1])[0]
    s.close()


# ---- 2. tile edges -------------------------------------------------------------------------------------------------------------
def mix(rng, parts, dim):
    """a row with about the given cosines to the given (nearly orthogonal) vectors, at a random length"""
    v = np.zeros(dim, dtype=np.float64)
    u = rng.standard_normal(dim)
    for cos, vec in parts:  # (the vectors are orthogonal: edge_case)
        e = vec.astype(np.float64) / np.linalg.norm(vec.astype(np.float64))
        v += cos * e
        u -= (u @ e) * e
    rest = max(0.0, 1.0 - sum(c * c for c, _ in parts))
    v += np.sqrt(rest) * u / np.linalg.norm(u)
    return (v * rng.uniform(0.5, 2.0)).astype(np.float32)


def edge_case(dim, K, tile, n=800):
    """rows 0..19: best the last label of tile 0, second the first of tile 1; rows 20..39: the other way round; rows 40..59: the two
    best in tile 0 (labels 3 and 7), the third alone in tile 1"""
    rng = np.random.default_rng(2000 + dim + K)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    labels = rng.standard_normal((K, dim)).astype(np.float32)
    special = [3, 7, tile - 1, tile]  # made orthogonal to each other, so that a planted row's cosines are the planted ones
    for i, j in enumerate(special):
        v = labels[j].astype(np.float64)
        for k in special[:i]:
            e = labels[k].astype(np.float64)
            v -= (v @ e) / (e @ e) * e
        labels[j] = v.astype(np.float32)
    for r in range(min(n, 60)):
        if r < 20:
            rows[r] = mix(rng, [(0.7, labels[tile - 1]), (0.5, labels[tile])], dim)
        elif r < 40:
            rows[r] = mix(rng, [(0.5, labels[tile - 1]), (0.7, labels[tile])], dim)
        else:
            rows[r] = mix(rng, [(0.6, labels[3]), (0.5, labels[7]), (0.4, labels[tile])], dim)
    return np.ascontiguousarray(rows), make_ids(rng, n), labels


def check_edges(got, n, tile):
    lab = got[0]
    assert (lab[: min(n, 20), :2] == [tile - 1, tile]).all()
    assert (lab[20 : min(n, 40), :2] == [tile, tile - 1]).all()
    if lab.shape[1] >= 3:
        assert (lab[40 : min(n, 60), :3] == [3, 7, tile]).all()


@pytest.mark.parametrize("shape", [(384, 129, 128), (640, 65, 64), (1280, 33, 32)])
def test_tile_edges(ctx, oracle, shape):
    dim, K, tile = shape
    rows, ids, labels = edge_case(dim, K, tile)
    s = build(ctx, rows, ids)
    for m in (2, 3):
        got = s.assign_top(None, labels, m)
        check_assign_top(got, assign_top_reference(oracle, rows, labels, m), ids)
        check_edges(got, len(ids), tile)
        st = s.last_assign_top_stats()
        assert st["tile_labels"] == tile and st["label_tiles"] == 2 and st["reruns"] == 0 and st["m"] == m
    s.close()


@pytest.mark.parametrize("n", [1, 31, 33])
def test_few_rows(ctx, oracle, n):
    rows, ids, labels = edge_case(D, 129, 128, n)
    s = build(ctx, rows, ids)
    got = s.assign_top(None, labels, 2)
    check_assign_top(got, assign_top_reference(oracle, rows, labels, 2), ids)
    check_edges(got, n, 128)
    s.close()


# ---- 3. ties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_ties(ctx, oracle, metric):
    rng = np.random.default_rng(31)
    n, K, tile = 300, 130, 128
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    labels = rng.standard_normal((K, D)).astype(np.float32)
    labels[10] = labels[40] = labels[90] = neighbour(rng, rows[0], 0.9)   # three bit-identical labels: the two lower ones
    labels[tile - 1] = labels[tile] = neighbour(rng, rows[1], 0.9)        # identical labels on both sides of the tile edge
    labels[K - 1] = labels[20] = neighbour(rng, rows[2], 0.7)             # a copy of the second best at K - 1 loses
    labels[5] = neighbour(rng, rows[2], 0.9)
    s = build(ctx, rows, ids, metric)
    got = s.assign_top(None, labels, 2)
    check_assign_top(got, assign_top_reference(oracle, rows, labels, 2, None, metric), ids)
    assert list(got[0][0]) == [10, 40] and bits(got[1][0])[0] == bits(got[1][0])[1]
    assert list(got[0][1]) == [tile - 1, tile] and bits(got[1][1])[0] == bits(got[1][1])[1]
    assert list(got[0][2]) == [5, 20]
    got3 = s.assign_top(None, labels, 3)
    check_assign_top(got3, assign_top_reference(oracle, rows, labels, 3, None, metric), ids)
    assert list(got3[0][0]) == [10, 40, 90] and list(got3[0][2]) == [5, 20, K - 1]
    s.close()


# ---- 4. the score bound --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_bound_is_exact(ctx, oracle, metric):
    """Rows of 16 ones (|x| = 4) and labels of 4 ones (|l| = 2) that share t features: the dot is t and the cosine t / 8, exact in
    every arithmetic.  The bound is c >= (double)min_score: the float of an actual c is included, the next float above excluded."""
    rng = np.random.default_rng(41)
    n, K = 64, 5
    rows = np.zeros((n, D), dtype=np.float32)
    labels = np.zeros((K, D), dtype=np.float32)
    for r in range(n):
        rows[r, 16 * (r % 8) : 16 * (r % 8) + 16] = 1.0
    for j in range(K):  # label j shares j features with the rows that start at feature 0
        labels[j, :j] = 1.0
        labels[j, 200 + 4 * j : 200 + 4 * j + 4 - j] = 1.0
    ids = make_ids(rng, n)
    mode = 1 if metric == "dot" else 0
    c = [oracle.canonical_score(labels[j], rows[0], mode) for j in range(K)]
    assert c == ([0.0, 1.0, 2.0, 3.0, 4.0] if metric == "dot" else [0.0, 0.125, 0.25, 0.375, 0.5])
    s = build(ctx, rows, ids, metric)
    for j in (1, 2, 3):
        at = np.float32(c[j])
        above = np.nextafter(at, np.float32(np.inf))
        for bound, kept in ((at, [4, 3, 2, 1][: 5 - j]), (above, [4, 3, 2, 1][: 4 - j])):
            got = s.assign_top(None, labels, 8, bound)
            check_assign_top(got, assign_top_reference(oracle, rows, labels, 8, bound, metric), ids)
            assert list(got[0][0, : got[3][0]]) == kept and list(got[0][8, : got[3][8]]) == kept
    high = s.assign_top(None, labels, 3, 2.0 if metric == "cosine" else 1e9)  # above every score: nothing is listed
    assert (high[3] == 0).all() and (high[0] == -1).all() and np.isnan(high[1]).all() and (high[4] == 0).all()
    np.testing.assert_array_equal(high[2], ids)
    s.close()


def test_bound_shortens_the_list(ctx, oracle):
    rng = np.random.default_rng(42)
    n, K, pairs, bound = 1000, 37, 20, 0.5
    rows = rng.standard_normal((n, D)).astype(np.float32)
    labels = rng.standard_normal((K, D)).astype(np.float32)
    for i in range(pairs):
        rows[37 * i + 5] = neighbour(rng, labels[i % K], 0.8) * np.float32(rng.uniform(0.5, 2.0))
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids)
    got = s.assign_top(None, labels, 4, bound)
    check_assign_top(got, assign_top_reference(oracle, rows, labels, 4, bound), ids)
    assert got[3].sum() == pairs and got[3].max() == 1
    # listed => s + mg >= min_score - margin => s >= min_score - 2 margin => c >= min_score - 3 margin: the list rule, not a measurement
    G = (rows.astype(np.float64) @ labels.astype(np.float64).T) / np.outer(np.sqrt(canonical_norms(rows)), np.sqrt(canonical_norms(labels)))
    allowed = int((G >= bound - 3 * margin(D)).sum())
    st = s.last_assign_top_stats()
    print("candidates %d allowed %d" % (st["candidates"], allowed))
    assert pairs <= st["candidates"] <= allowed and allowed < 2 * pairs
    # without the bound every row lists at least one candidate
    s.assign_top(None, labels, 4)
    assert s.last_assign_top_stats()["candidates"] >= 4 * n
    s.close()


# ---- 5. rows that take no part, wild rows and labels ---------------------------------------------------------------------------
def test_rows_that_take_no_part_and_wild_ones(ctx, oracle):
    rng = np.random.default_rng(51)
    n, K, m = 300, 20, 3
    rows = rng.standard_normal((n, D)).astype(np.float32)
    labels = rng.standard_normal((K, D)).astype(np.float32)
    rows[5] = 0.0
    labels[7] = 0.0
    rows[6, 17] = np.nan  # a row without a finite norm: unsearchable, it takes no part
    scales = [2.0 ** -60, 2.0 ** -21, 2.0 ** 21, 2.0 ** 60]  # norms of about that: outside the certified range of the f32 screen
    for i, sc in enumerate(scales):  # rows 100.. are rows 10.. times a power of two: the same cosines
        rows[100 + i] = rows[10 + i] * np.float32(sc / 16.0)
        rows[10 + i] = rows[10 + i] * np.float32(1.0 / 16.0)
    ids = make_ids(rng, n)
    live = np.ones(n, dtype=bool)
    live[6] = False
    s = build(ctx, rows, ids)
    got = s.assign_top(None, labels, m)
    check_assign_top(got, assign_top_reference(oracle, rows, labels, m, None, "cosine", live), ids)
    assert (got[3][[5, 6]] == 0).all() and (got[0][[5, 6]] == -1).all() and np.isnan(got[1][[5, 6]]).all() and (np.delete(got[3], [5, 6]) == m).all()
    assert (got[0] != 7).all() and got[4][7] == 0  # the zero label is never listed
    for i in range(len(scales)):
        np.testing.assert_array_equal(got[0][100 + i], got[0][10 + i])
        np.testing.assert_array_equal(bits(got[1][100 + i]), bits(got[1][10 + i]))
    # wild labels: the same labels at 2^-21 and 2^21 of unit length give the same lists
    unit = (labels.astype(np.float64) / np.maximum(np.linalg.norm(labels.astype(np.float64), axis=1, keepdims=True), 1e-300)).astype(np.float32)
    base = s.assign_top(None, unit, m)
    check_assign_top(base, assign_top_reference(oracle, rows, unit, m, None, "cosine", live), ids)
    for sc in (2.0 ** -21, 2.0 ** 21):
        wild = (unit * np.float32(sc)).astype(np.float32)
        again = s.assign_top(None, wild, m)
        same(again, base)
    # one wild label among certified ones, and a bound
    one = unit.copy()
    one[3] = unit[3] * np.float32(2.0 ** 21)
    got1 = s.assign_top(None, one, m, 0.05)
    check_assign_top(got1, assign_top_reference(oracle, rows, one, m, 0.05, "cosine", live), ids)
    # hidden rows: nothing while hidden, back afterwards
    hidden = [20, 21, 150]
    s.hide_items(ids[hidden])
    part = live.copy()
    part[hidden] = False
    h = s.assign_top(None, labels, m)
    check_assign_top(h, assign_top_reference(oracle, rows, labels, m, None, "cosine", part), ids)
    assert (h[3][hidden] == 0).all() and (h[0][hidden] == -1).all() and len(h[3]) == n
    s.unhide_items(ids[hidden])
    same(s.assign_top(None, labels, m), got)
    s.close()


def test_dot_rows_and_labels_without_a_cosine(ctx, oracle):
    """Under the dot metric a zero row and a zero label take part: c = 0, the lower labels first"""
    rng = np.random.default_rng(52)
    rows = rng.standard_normal((100, D)).astype(np.float32)
    rows[7] = 0.0
    labels = rng.standard_normal((6, D)).astype(np.float32)
    labels[4] = 0.0
    ids = make_ids(rng, 100)
    s = build(ctx, rows, ids, "dot")
    got = s.assign_top(None, labels, 3)
    check_assign_top(got, assign_top_reference(oracle, rows, labels, 3, None, "dot"), ids)
    assert list(got[0][7]) == [0, 1, 2] and (got[1][7] == 1.0).all() and (got[0] == 4).any()
    hidden = [7, 30]
    s.hide_items(ids[hidden])
    part = np.ones(100, dtype=bool)
    part[hidden] = False
    h = s.assign_top(None, labels, 3, 0.0)
    check_assign_top(h, assign_top_reference(oracle, rows, labels, 3, 0.0, "dot", part), ids)
    assert (h[3][hidden] == 0).all()
    s.close()


# ---- 6. list growth ------------------------------------------------------------------------------------------------------------
def test_overflow_rerun(ctx, oracle):
    rng = np.random.default_rng(61)
    n, K = 800, 129
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    one = rng.standard_normal((1, D)).astype(np.float32)
    labels = (one + np.float32(1e-4) * rng.standard_normal((K, D)).astype(np.float32)).astype(np.float32)  # every label a candidate of every row
    s = build(ctx, rows, ids)
    got = s.assign_top(None, labels, 2)
    st = s.last_assign_top_stats()
    print(st)
    assert st["candidates"] == n * K == 103200 and st["candidates"] > 65536 and st["reruns"] == 1 and st["label_tiles"] == 2
    check_assign_top(got, assign_top_reference(oracle, rows, labels, 2), ids)
    s.close()


# ---- 7. segments, source lists, views ------------------------------------------------------------------------------------------
def test_segments_sources_and_views(ctx, oracle):
    rng = np.random.default_rng(71)
    sizes = [64, 96, 32, 1, 128, 5, 300]  # (a piece that is not the last of its source is a whole number of blocks: test_assign_gpu.py)
    src_of = [1, 2, 3, 1, 2, 3, 2]
    n = sum(sizes)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    labels = rng.standard_normal((11, D)).astype(np.float32)
    s = pa.Searcher(ctx, D, "cosine")
    first = np.concatenate([[0], np.cumsum(sizes)])
    where = {1: [], 2: [], 3: []}
    for i, sid in enumerate(src_of):
        s.reserve(sid, sizes[i])
        s.add_rows(sid, rows[first[i] : first[i + 1]], ids[first[i] : first[i + 1]])
        s.finalize()
        where[sid] += list(range(first[i], first[i + 1]))
    assert s.num_segments == 7 and s.num_rows == n

    def rows_of(sources):
        return np.array([r for sid in (1, 2, 3) if sid in sources for r in where[sid]], dtype=np.int64)

    for sources in (None, [3, 1, 2], [2], [3, 1]):
        sel = rows_of([1, 2, 3] if sources is None else sources)
        got = s.assign_top(sources, labels, 3, 0.02)
        check_assign_top(got, assign_top_reference(oracle, rows[sel], labels, 3, 0.02), ids[sel])
    empty = s.assign_top([], labels, 3)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and len(empty[2]) == 0 and len(empty[3]) == 0 and (empty[4] == 0).all()
    assert len(s.assign_top([99], labels, 3)[2]) == 0
    # the count-only form, and outputs that are too short: PCV_ERR_INVALID with out_n set
    L, got_n = _ffi.lib(), C.c_int64(-1)
    src = (C.c_int64 * 2)(3, 1)
    assert L.pcv_searcher_assign_top(s._handle, _ffi.f32p(labels), 11, 3, 0.0, src, 2, 0, None, None, None, None, None, C.byref(got_n)) == 0
    assert got_n.value == len(rows_of([3, 1]))
    out, cnt, got_n = np.zeros((10, 3), dtype=np.int32), np.zeros(10, dtype=np.int32), C.c_int64(-1)
    assert L.pcv_searcher_assign_top(s._handle, _ffi.f32p(labels), 11, 3, 0.0, src, 2, 10, _ffi.i32p(out), None, None, _ffi.i32p(cnt), None, C.byref(got_n)) == 1
    assert got_n.value == len(rows_of([3, 1])) and b"room for 10" in L.pcv_last_error()
    # NULL scores, ids and label_rows are allowed
    room = int(got_n.value)
    out, cnt = np.zeros((room, 3), dtype=np.int32), np.zeros(room, dtype=np.int32)
    assert L.pcv_searcher_assign_top(s._handle, _ffi.f32p(labels), 11, 3, 0.0, src, 2, room, _ffi.i32p(out), None, None, _ffi.i32p(cnt), None, C.byref(got_n)) == 0
    full = s.assign_top([3, 1], labels, 3, 0.0)
    np.testing.assert_array_equal(out, full[0])
    np.testing.assert_array_equal(cnt, full[3])
    # a view equals a fresh searcher of its rows
    sel = rows_of([1, 2, 3])
    allowed = sel[rng.random(n) < 0.4]
    v = s.view(ids[allowed])
    fresh = build(ctx, rows[allowed], ids[allowed])
    a, b = v.assign_top(None, labels, 2), fresh.assign_top(None, labels, 2)
    same(a, b)
    check_assign_top(a, assign_top_reference(oracle, rows[allowed], labels, 2), ids[allowed])
    v.close()
    fresh.close()
    s.close()


# ---- 8. independence of the search settings, no pass state touched -------------------------------------------------------------
def test_independent_of_search_settings(ctx, oracle):
    rng = np.random.default_rng(81)
    n, K, m = 700, 40, 3
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    labels = rng.standard_normal((K, D)).astype(np.float32)
    want = assign_top_reference(oracle, rows, labels, m, 0.0)
    for copy, kernel in (("off", "auto"), ("int8", "auto"), ("auto", "auto"), ("auto", "wave")):
        s = pa.Searcher(ctx, D, "cosine")
        s.set_screening_copy(copy)
        s.add_rows(1, rows, ids)
        s.finalize()
        s.set_kernel(kernel)
        before_a, before_s = s.assign(None, labels), s.search_vectors(None, 10, labels[:5])
        check_assign_top(s.assign_top(None, labels, m, 0.0), want, ids)
        same(s.assign(None, labels), before_a)
        same(s.search_vectors(None, 10, labels[:5]), before_s)
        s.close()


# ---- 9. the rows per label -----------------------------------------------------------------------------------------------------
def test_label_rows_is_the_histogram_of_the_lists(ctx):
    rng = np.random.default_rng(91)
    n, K = 500, 9
    rows = rng.standard_normal((n, D)).astype(np.float32)
    labels = rng.standard_normal((K, D)).astype(np.float32)
    s = build(ctx, rows, make_ids(rng, n))
    for m, bound in ((1, None), (4, None), (8, 0.0), (8, 0.05)):
        lab, score, ids, counts, label_rows = s.assign_top(None, labels, m, bound)
        np.testing.assert_array_equal(label_rows, np.bincount(lab[lab >= 0], minlength=K))
        np.testing.assert_array_equal(counts, (lab >= 0).sum(axis=1))
        assert s.last_assign_top_stats()["listed"] == counts.sum() == label_rows.sum()
        listed = np.arange(lab.shape[1])[None, :] < counts[:, None]
        assert ((lab >= 0) == listed).all() and (np.isnan(score) == ~listed).all()  # the unused slots are behind the used ones
    s.close()


def test_errors_on_the_device(ctx):
    s = build(ctx, np.ones((40, D), dtype=np.float32), np.arange(40, dtype=np.int64))
    bad = np.ones((3, D), dtype=np.float32)
    for v in (np.nan, np.inf, -np.inf):
        bad[1, 17] = v
        with pytest.raises(pa.PcvError) as e:
            s.assign_top(None, bad, 2)
        assert e.value.status == 1 and "label 1" in str(e.value)
    for m in (0, 9):
        with pytest.raises(pa.PcvError) as e:
            s.assign_top(None, np.ones((3, D), dtype=np.float32), m)
        assert e.value.status == 1
    with pytest.raises(pa.PcvError) as e:
        s.assign_top(None, np.ones((3, D), dtype=np.float32), 2, float("nan"))
    assert e.value.status == 1
    s.add_rows(1, np.ones((1, D), dtype=np.float32), np.array([99], dtype=np.int64))  # pending rows: as a search
    with pytest.raises(pa.PcvError):
        s.assign_top(None, np.ones((3, D), dtype=np.float32), 2)
    s.close()


# ---- 10. the C++ mirror --------------------------------------------------------------------------------------------------------
def test_cpp_mirror_assign_top_program():
    src = os.path.join(ROOT, "tests", "cpp", "assign_top_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "assign_top_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "assign_top_mirror_test: ok" in r.stdout
