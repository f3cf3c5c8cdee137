"""GPU: item labels (pcv_searcher_assign, _label_sums, _kmeans), through the Python mirror of the C ABI.  The reference of every
check is assign_ref.py: the oracle's canonical score of every (label, row) that can be the row's best, argmax with ties to the lower
label; labels, f32 score bits, ids and counts are compared for equality."""
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from assign_ref import assign_reference, bits, check_assign, kmeans_reference, sums_reference
from duplicates_ref import build, make_ids, neighbour, screen_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384


def margin(dim):
    """selfjoin_margin at the padded dimension (selfjoin_kernels.hip)"""
    dp = (dim + 63) // 64 * 64
    return 0.00783 + 1.02 * ((dp + 16) * 1.2e-7) + 1e-6


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
        got = s.assign(None, labels)
        want = assign_reference(oracle, rows, labels, metric)
        check_assign(got, want, ids)
        st = s.last_assign_stats()
        assert st["rows"] == n and st["label_tiles"] == 1 and st["tile_labels"] == 128 and st["candidates"] >= (want[0] >= 0).sum()
        assert got[0][3] == K // 2 or metric == "dot"
        # the scores are those of a search with the labels as queries, for the same pairs
        s_ids, s_scores, s_counts = s.search_vectors(None, n, labels)
        for j in range(K):
            at = {int(i): p for p, i in enumerate(s_ids[j, : s_counts[j]].tolist())}
            mine = np.nonzero(got[0] == j)[0]
            np.testing.assert_array_equal(bits(got[1][mine]), bits(s_scores[j, [at[int(ids[r])] for r in mine]]))
    s.close()


# ---- 2. tile edges -------------------------------------------------------------------------------------------------------------
def planted_case(dim, K, tile, n=800):
    """rows 0..39 are near the last label of the first tile, rows 40..79 near the only label of the second one (if there is one)"""
    rng = np.random.default_rng(1000 + dim + K)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    labels = rng.standard_normal((K, dim)).astype(np.float32)
    last = min(K, tile) - 1
    for r in range(0, min(40, n)):
        rows[r] = neighbour(rng, labels[last], 0.8) * np.float32(rng.uniform(0.5, 2.0))
    if K > tile:
        for r in range(40, min(80, n)):
            rows[r] = neighbour(rng, labels[tile], 0.8) * np.float32(rng.uniform(0.5, 2.0))
    return np.ascontiguousarray(rows), make_ids(rng, n), labels, last


@pytest.mark.parametrize("shape", [(384, 128, 128), (384, 129, 128), (640, 64, 64), (640, 65, 64), (1280, 33, 32)])
def test_tile_edges(ctx, oracle, shape):
    dim, K, tile = shape
    rows, ids, labels, last = planted_case(dim, K, tile)
    s = build(ctx, rows, ids)
    got = s.assign(None, labels)
    check_assign(got, assign_reference(oracle, rows, labels), ids)
    assert (got[0][:40] == last).all() and (K <= tile or (got[0][40:80] == tile).all())
    st = s.last_assign_stats()
    assert st["tile_labels"] == tile and st["label_tiles"] == (K + tile - 1) // tile and st["reruns"] == 0
    s.close()


@pytest.mark.parametrize("n", [1, 31, 33])
def test_few_rows(ctx, oracle, n):
    rows, ids, labels, last = planted_case(D, 129, 128, n)
    s = build(ctx, rows, ids)
    got = s.assign(None, labels)
    check_assign(got, assign_reference(oracle, rows, labels), ids)
    assert (got[0][: min(n, 40)] == last).all()
    s.close()


# ---- 3. ties and near ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_ties(ctx, oracle, metric):
    rng = np.random.default_rng(31)
    n = 300
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    base = rng.standard_normal((4, D)).astype(np.float32)
    # two identical labels; a label, its copy times 2 and times 2^-3 (cosine: the same score bits)
    labels = np.stack([base[0], base[1], base[1], base[2], base[3], base[3] * np.float32(2.0), base[3] * np.float32(0.125)])
    s = build(ctx, rows, ids, metric)
    got = s.assign(None, labels)
    check_assign(got, assign_reference(oracle, rows, labels, metric), ids)
    assert (got[0] != 2).all() and (got[0] == 1).any()
    if metric == "cosine":
        assert (got[0] < 5).all() and (got[0] == 4).any()
    s.close()


def test_near_ties(ctx, oracle):
    rng = np.random.default_rng(32)
    n, pairs = 200, 40
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    labels = np.empty((2 * pairs, D), dtype=np.float32)
    for i in range(pairs):  # row i: two labels whose cosines differ by about 1e-7, the better one first or second
        lo, hi = neighbour(rng, rows[i], 0.9), neighbour(rng, rows[i], 0.9 + 1e-7)
        labels[2 * i], labels[2 * i + 1] = (lo, hi) if i % 2 else (hi, lo)
    gap = np.array([abs(oracle.canonical_score(labels[2 * i], rows[i]) - oracle.canonical_score(labels[2 * i + 1], rows[i])) for i in range(pairs)])
    print("gaps: median %.3g max %.3g" % (np.median(gap), gap.max()))
    assert gap.max() < 1e-6
    s = build(ctx, rows, ids)
    got = s.assign(None, labels)
    want = assign_reference(oracle, rows, labels)
    check_assign(got, want, ids)
    assert all(got[0][i] in (2 * i, 2 * i + 1) for i in range(pairs))
    first = sum(int(got[0][i] == 2 * i) for i in range(pairs))
    assert 5 <= first <= pairs - 5  # both orders occur
    s.close()


# ---- 4. the edge of the margin -------------------------------------------------------------------------------------------------
DOWN = 1.0 + 2.0 ** -8 - 2.0 ** -18  # exact in f32; rounds down to 1 in bf16
UP = 1.0 + 2.0 ** -8 + 2.0 ** -18    # rounds up to 1 + 2^-7


def hostile_case(oracle, dim, n_rows=24):
    """Row x: features +-2^e DOWN.  Label A = x: cosine 1, but both bf16 roundings go down, the screen sees 1 - u (2 + u).  Label B:
    the same signs and exponents with mantissa UP (the roundings of x and B cancel) and one small feature doubled: its cosine is
    just below 1 and the screen sees it nearly unchanged.  So the true best has the lower screening score by nearly the whole bf16
    part of the margin: the gap is about 0.0077, between 0.95 m and m.  The candidate test lets the true best through iff the gap is
    at most twice the margin in use, so what this input detects is a margin below gap / 2, about 0.48 m — a screen without a margin,
    or with the accumulation or rinv terms alone.  A margin of exactly m / 2 still passes it: one row rounds all its features one
    way, and the roundings of the row then cancel in one of the two labels, which caps the gap at about m.
    A before B for even rows, B before A for odd ones."""
    rng = np.random.default_rng(400 + dim)
    rows = rng.standard_normal((200, dim)).astype(np.float32)
    labels, truth = [], {}
    places = rng.permutation(200)[:n_rows]
    for i, r in enumerate(places):
        e = rng.integers(-2, 2, size=dim)
        e[0] = -3
        sign = rng.choice([-1.0, 1.0], size=dim)
        x = (sign * np.ldexp(DOWN, e)).astype(np.float32)
        e2 = e.copy()
        e2[0] = -2
        b = (sign * np.ldexp(UP, e2)).astype(np.float32)
        rows[r] = x
        if i % 2 == 0:
            ja, jb = len(labels), len(labels) + 1
            labels += [x.copy(), b]
        else:
            jb, ja = len(labels), len(labels) + 1
            labels += [b, x.copy()]
        truth[int(r)] = (ja, jb)
    labels = np.ascontiguousarray(np.stack(labels + [rng.standard_normal(dim).astype(np.float32) for _ in range(5)]))
    m = margin(dim)
    for r, (ja, jb) in truth.items():
        ca, cb = oracle.canonical_score(labels[ja], rows[r]), oracle.canonical_score(labels[jb], rows[r])
        sa, sb = screen_score(labels[ja], rows[r]), screen_score(labels[jb], rows[r])
        assert ca > cb, (ca, cb)
        assert sa < sb - m / 2, (sa, sb, m)  # the true best has the lower screening score by more than half the margin
        assert 0.95 * m < sb - sa < 2 * m, (sa, sb, m)  # ... in fact by nearly the whole of it
    return np.ascontiguousarray(rows), labels, truth


@pytest.mark.parametrize("dim", [64, 384, 768])
def test_edge_of_the_margin(ctx, oracle, dim):
    rows, labels, truth = hostile_case(oracle, dim)  # (asserts on the CPU before the device is used)
    ids = make_ids(np.random.default_rng(dim), rows.shape[0])
    s = build(ctx, rows, ids)
    got = s.assign(None, labels)
    check_assign(got, assign_reference(oracle, rows, labels), ids)
    for r, (ja, _jb) in truth.items():
        assert got[0][r] == ja
    s.close()


# ---- 5. rows that take no part, wild rows --------------------------------------------------------------------------------------
def test_rows_that_take_no_part_and_wild_rows(ctx, oracle):
    rng = np.random.default_rng(51)
    n, K = 300, 20
    rows = rng.standard_normal((n, D)).astype(np.float32)
    labels = rng.standard_normal((K, D)).astype(np.float32)
    rows[5] = 0.0
    scales = [2.0 ** -63, 2.0 ** -20, 2.0 ** 20, 2.0 ** 60]
    for i, sc in enumerate(scales):  # rows 100.. are rows 10.. times a power of two: the same cosines
        rows[100 + i] = rows[10 + i] * np.float32(sc)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids)
    got = s.assign(None, labels)
    check_assign(got, assign_reference(oracle, rows, labels), ids)
    assert got[0][5] == -1 and np.isnan(got[1][5]) and (np.delete(got[0], 5) >= 0).all()
    for i in range(len(scales)):
        assert got[0][100 + i] == got[0][10 + i] and bits(got[1][100 + i : 101 + i]) == bits(got[1][10 + i : 11 + i])
    # wild labels: the same labels at 2^-30 and 2^30 of their length
    for sc in (2.0 ** -30, 2.0 ** 30):
        wild = (labels * np.float32(sc)).astype(np.float32)
        again = s.assign(None, wild)
        np.testing.assert_array_equal(again[0], got[0])
        np.testing.assert_array_equal(bits(again[1]), bits(got[1]))
    # hidden rows: -1 while hidden, back afterwards
    hidden = [20, 21, 150]
    s.hide_items(ids[hidden])
    part = np.ones(n, dtype=bool)
    part[hidden] = False
    part[5] = True
    h = s.assign(None, labels)
    check_assign(h, assign_reference(oracle, rows, labels, "cosine", part), ids)
    assert (h[0][hidden] == -1).all() and np.isnan(h[1][hidden]).all() and len(h[0]) == n
    s.unhide_items(ids[hidden])
    check_assign(s.assign(None, labels), assign_reference(oracle, rows, labels), ids)
    # removed rows: n shrinks
    gone = [0, 33, 299]
    s.remove_items(ids[gone])
    keep = np.setdiff1d(np.arange(n), gone)
    r = s.assign(None, labels)
    assert len(r[0]) == n - 3
    check_assign(r, assign_reference(oracle, rows[keep], labels), ids[keep])
    s.close()


def test_dot_rows_without_a_cosine(ctx, oracle):
    """Under the dot metric a zero row takes part: every product is 0, the first label wins at distance 1"""
    rng = np.random.default_rng(52)
    rows = rng.standard_normal((100, D)).astype(np.float32)
    rows[7] = 0.0
    labels = rng.standard_normal((6, D)).astype(np.float32)
    labels[4] = 0.0  # the zero label: c = 0 for every row
    ids = make_ids(rng, 100)
    s = build(ctx, rows, ids, "dot")
    got = s.assign(None, labels)
    check_assign(got, assign_reference(oracle, rows, labels, "dot"), ids)
    assert got[0][7] == 0 and got[1][7] == 1.0
    s.close()


# ---- 6. segments, source lists, views ------------------------------------------------------------------------------------------
def test_segments_sources_and_views(ctx, oracle):
    rng = np.random.default_rng(61)
    # seven pieces in three sources, added in turn, each announced (reserve) so that it gets a segment of its own: a piece that is not
    # the last of its source is a whole number of 32-row blocks, or the next add of that source would start in its spare rows
    sizes = [64, 96, 32, 1, 128, 5, 300]
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
    assert s.num_segments == 7 and s.num_rows == n  # 64, 1 | 96, 128, 300 | 32, 5 rows

    def rows_of(sources):  # in global position order: by source, in the order the sources were created
        return np.array([r for sid in (1, 2, 3) if sid in sources for r in where[sid]], dtype=np.int64)

    for sources in (None, [1, 2, 3], [3, 1, 2], [2], [3, 1], [1]):
        sel = rows_of([1, 2, 3] if sources is None else sources)
        got = s.assign(sources, labels)
        check_assign(got, assign_reference(oracle, rows[sel], labels), ids[sel])
    empty = s.assign([], labels)
    assert len(empty[0]) == 0 and len(empty[1]) == 0 and len(empty[2]) == 0 and (empty[3] == 0).all()
    assert len(s.assign([99], labels)[0]) == 0
    # a view equals a fresh searcher of its rows
    sel = rows_of([1, 2, 3])
    allowed = sel[rng.random(n) < 0.4]
    v = s.view(ids[allowed])
    fresh = build(ctx, rows[allowed], ids[allowed])
    a, b = v.assign(None, labels), fresh.assign(None, labels)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
    check_assign(a, assign_reference(oracle, rows[allowed], labels), ids[allowed])
    km_v, km_f = v.kmeans(None, 3, labels[:3], 2), fresh.kmeans(None, 3, labels[:3], 2)
    np.testing.assert_array_equal(bits(km_v[0]), bits(km_f[0]))
    np.testing.assert_array_equal(km_v[1], km_f[1])
    v.close()
    fresh.close()
    s.close()


# ---- 7. list growth ------------------------------------------------------------------------------------------------------------
def test_list_growth(ctx, oracle):
    rng = np.random.default_rng(71)
    n, K = 2000, 64
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    labels = np.repeat(rng.standard_normal((1, D)).astype(np.float32), K, axis=0)  # every label a candidate of every row
    s = build(ctx, rows, ids)
    got = s.assign(None, labels)
    st = s.last_assign_stats()
    print(st)
    assert st["candidates"] == n * K and st["candidates"] > max(65536, 4 * n) and st["reruns"] == 1
    check_assign(got, assign_reference(oracle, rows, labels), ids)
    assert (got[0] == 0).all()
    s.close()


# ---- 8. independence of the search settings ------------------------------------------------------------------------------------
def test_independent_of_search_settings(ctx, oracle):
    rng = np.random.default_rng(81)
    n, K = 700, 40
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    labels = rng.standard_normal((K, D)).astype(np.float32)
    want = assign_reference(oracle, rows, labels)
    for copy, kernel in (("off", "auto"), ("int8", "auto"), ("auto", "auto"), ("auto", "wave")):
        s = pa.Searcher(ctx, D, "cosine")
        s.set_screening_copy(copy)
        s.add_rows(1, rows, ids)
        s.finalize()
        s.set_kernel(kernel)
        check_assign(s.assign(None, labels), want, ids)
        s.close()


# ---- 9. k-means ----------------------------------------------------------------------------------------------------------------
def test_kmeans_planted_clusters(ctx, oracle):
    rng = np.random.default_rng(91)
    dim, per = 64, 200
    centres = rng.standard_normal((3, dim)).astype(np.float32)
    truth = np.repeat(np.arange(3), per)
    order = rng.permutation(3 * per)
    truth = truth[order]
    rows = np.stack([neighbour(rng, centres[t], 0.9) * np.float32(rng.uniform(0.5, 2.0)) for t in truth]).astype(np.float32)
    ids = make_ids(rng, 3 * per)
    s = build(ctx, rows, ids)
    seeds = [int(ids[np.nonzero(truth == t)[0][0]]) for t in range(3)]  # one item of each cluster, by id
    cent, label, score, got_ids, counts, iters, moved = s.kmeans(None, 3, seeds, max_iters=10)
    np.testing.assert_array_equal(label, truth)
    np.testing.assert_array_equal(counts, [per, per, per])
    np.testing.assert_array_equal(got_ids, ids)
    assert moved[-1] == 0 and len(moved) == iters + 1 and 1 <= iters < 10 and moved[0] == 3 * per
    w = kmeans_reference(oracle, rows, np.stack([rows[np.nonzero(truth == t)[0][0]] for t in range(3)]), 10)
    np.testing.assert_array_equal(bits(cent), bits(w[0]))
    np.testing.assert_array_equal(label, w[1])
    np.testing.assert_array_equal(bits(score), bits(w[2]))
    assert iters == w[4]
    np.testing.assert_array_equal(moved, w[5])
    s.close()


def test_kmeans_golden_bit_for_bit(ctx, oracle, golden_dir):
    g = np.load(os.path.join(golden_dir, "scan_n1000_d384.npz"))
    rows = np.ascontiguousarray(g["corpus"], dtype=np.float32)
    rng = np.random.default_rng(92)
    ids = make_ids(rng, rows.shape[0])
    init = rows[rng.permutation(rows.shape[0])[:8]].copy()
    s = build(ctx, rows, ids)
    cent, label, score, got_ids, counts, iters, moved = s.kmeans(None, 8, init, max_iters=5)
    w = kmeans_reference(oracle, rows, init, 5)
    np.testing.assert_array_equal(bits(cent), bits(w[0]))
    np.testing.assert_array_equal(label, w[1])
    np.testing.assert_array_equal(bits(score), bits(w[2]))
    np.testing.assert_array_equal(counts, w[3])
    assert iters == w[4] == 5
    np.testing.assert_array_equal(moved, w[5])
    # the sums on their own, for the final labels
    S, members = s.label_sums(None, label, 8)
    wS, wm = sums_reference(rows, label, 8)
    np.testing.assert_array_equal(S, wS)
    np.testing.assert_array_equal(members, wm)
    # a hidden row adds nothing and is not counted, whatever label it is given
    hidden = [4, 600]
    s.hide_items(ids[hidden])
    part = np.ones(rows.shape[0], dtype=bool)
    part[hidden] = False
    assert (label[hidden] >= 0).all()
    S, members = s.label_sums(None, label, 8)
    wS, wm = sums_reference(rows, label, 8, part)
    np.testing.assert_array_equal(S, wS)
    np.testing.assert_array_equal(members, wm)
    assert members.sum() == wm.sum() == (label >= 0).sum() - 2
    s.close()


def test_kmeans_empty_label_zero_iterations_and_dot(ctx, oracle):
    rng = np.random.default_rng(93)
    n = 400
    # every row and every other centroid lies on the side of the all-ones direction; label 3 points the other way and never wins
    rows = (rng.standard_normal((n, D)) + 0.5).astype(np.float32)
    rows = np.ascontiguousarray(rows * rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32))
    ids = make_ids(rng, n)
    init = (rng.standard_normal((5, D)) + 0.5).astype(np.float32)
    init[3] = -1.0
    assert (rows.astype(np.float64).sum(axis=1) > 0).all()
    s = build(ctx, rows, ids)
    cent, label, score, got_ids, counts, iters, moved = s.kmeans(None, 5, init, max_iters=3)
    assert counts[3] == 0 and (label != 3).all()
    np.testing.assert_array_equal(bits(cent[3]), bits(init[3]))  # a label without members keeps its vector
    w = kmeans_reference(oracle, rows, init, 3)
    np.testing.assert_array_equal(bits(cent), bits(w[0]))
    np.testing.assert_array_equal(label, w[1])
    # max_iters = 0 is assign
    z = s.kmeans(None, 5, init, max_iters=0)
    a = s.assign(None, init)
    np.testing.assert_array_equal(bits(z[0]), bits(init))
    np.testing.assert_array_equal(z[1], a[0])
    np.testing.assert_array_equal(bits(z[2]), bits(a[1]))
    np.testing.assert_array_equal(z[3], a[2])
    np.testing.assert_array_equal(z[4], a[3])
    assert z[5] == 0 and list(z[6]) == [int((a[0] >= 0).sum())]
    # a dot searcher clusters by cosine too
    sd = build(ctx, rows, ids, "dot")
    d = sd.kmeans(None, 5, init, max_iters=3)
    np.testing.assert_array_equal(bits(d[0]), bits(cent))
    np.testing.assert_array_equal(d[1], label)
    np.testing.assert_array_equal(bits(d[2]), bits(score))
    np.testing.assert_array_equal(d[6], moved)
    sd.close()
    s.close()


def test_errors_on_the_device(ctx):
    s = build(ctx, np.ones((40, D), dtype=np.float32), np.arange(40, dtype=np.int64))
    bad = np.ones((3, D), dtype=np.float32)
    for v in (np.nan, np.inf, -np.inf):
        bad[1, 17] = v
        with pytest.raises(pa.PcvError) as e:
            s.assign(None, bad)
        assert e.value.status == 1 and "label 1" in str(e.value)
    with pytest.raises(pa.PcvError) as e:
        s.label_sums(None, np.zeros(39, dtype=np.int32), 2)
    assert e.value.status == 1
    with pytest.raises(pa.PcvError) as e:
        s.label_sums(None, np.full(40, 2, dtype=np.int32), 2)
    assert e.value.status == 1
    s.add_rows(1, np.ones((1, D), dtype=np.float32), np.array([99], dtype=np.int64))  # pending rows: as a search
    with pytest.raises(pa.PcvError):
        s.assign(None, np.ones((3, D), dtype=np.float32))
    s.close()


# ---- 10. the C++ mirror --------------------------------------------------------------------------------------------------------
def test_cpp_mirror_assign_program():
    src = os.path.join(ROOT, "tests", "cpp", "assign_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "assign_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "assign_mirror_test: ok" in r.stdout
