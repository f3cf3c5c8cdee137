"""GPU: item neighbours (pcv_searcher_neighbors), through the Python mirror of the C ABI.  The reference of every check is
neighbors_ref.py: the oracle's canonical cosine of every partner that can be among a row's k best, sorted (-c, position); ids, counts
and the f32 bits of the scores are compared for equality.  Each test first asserts on the CPU what makes its input hostile."""
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from duplicates_ref import bf16_rne, build, make_ids, neighbour, screen_score
from neighbors_ref import bits, check, reference, takes_part

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
    if metric == "dot":  # rows of several lengths: the neighbours are by cosine all the same
        rows = (rows * rng.uniform(0.5, 1.5, size=(rows.shape[0], 1))).astype(np.float32)
    rows = np.ascontiguousarray(rows)
    n = rows.shape[0]
    ids = make_ids(rng, n)
    live = takes_part(rows)
    P = int(live.sum())
    assert P == n or name == "scan_n1000_d384"  # (the larger corpus has rows without a cosine)
    s = build(ctx, rows, ids, metric)
    for k in (1, 10, 64):
        got = s.neighbors(None, k)
        check(got, reference(oracle, rows, ids, k))
        assert (got[3][live] == min(k, P - 1)).all() and (got[3][~live] == 0).all()  # (n = 77: 76 partners, so min(k, 76))
        st = s.last_neighbor_stats()
        assert st["rows"] == n and st["k"] == k and st["listed"] == P * min(k, P - 1) and st["candidates"] >= st["listed"]
        assert st["tile_rows"] == 128 and st["sample_stride"] == 1 and st["reruns"] == 0
    s.close()


# ---- 2. the sampled bound pass -------------------------------------------------------------------------------------------------
def test_sampled_bound_pass_spans_and_partial_last_tile(ctx, oracle):
    """12 320 rows of 64 features are 385 blocks: every fourth is sampled (97 of them), in 49 spans of two, and the last tile has one
    block.  Owners in the first tile, in one in the middle and in the last one get 0.999-neighbours where the bound pass does not
    look (blocks 5 and 7), on both sides of a span cut (blocks 4 and 8, both sampled) and in their own tile."""
    rng = np.random.default_rng(22)
    n, dim, k = 12320, 64, 10
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    owners = [3, 97, 160 * 32 + 5, 162 * 32 + 31, 384 * 32 + 1, n - 1]
    planted = {}
    for i, r in enumerate(owners):
        own_tile = (r // 128) * 128
        spots = [5 * 32 + 2 * i, 7 * 32 + 2 * i, 4 * 32 + 10 + 2 * i, 8 * 32 + 10 + 2 * i, min(n - 1, own_tile + 40 + i) if r != own_tile + 40 + i else own_tile + 39]
        if own_tile + 32 >= n:
            spots[-1] = own_tile + 8 + i
        for j, p in enumerate(spots):
            rows[p] = neighbour(rng, rows[r], 0.999) * np.float32(rng.uniform(0.5, 2.0))
        planted[r] = spots
    ids = make_ids(rng, n)
    want = reference(oracle, rows, ids, k)
    for r, spots in planted.items():  # what is hostile: the planted rows are the owner's best five, and random rows are far below them
        assert set(want[1][r, :5].tolist()) == set(ids[spots].tolist()), r
        assert want[2][r, 4] > 0.99 and want[2][r, 5] < 0.7
    s = build(ctx, rows, ids)
    got = s.neighbors(None, k)
    st = s.last_neighbor_stats()
    print(st)
    assert st["sample_stride"] > 1 and st["spans"] > k and st["tile_rows"] == 128 and st["rows"] == n
    check(got, want)
    s.close()


# ---- 3. the edge of the 2 m slack ----------------------------------------------------------------------------------------------
DOWN = 1.0 + 2.0 ** -8 - 2.0 ** -18  # exact in f32; rounds down to 1 in bf16
UP = 1.0 + 2.0 ** -8 + 2.0 ** -18    # rounds up to 1 + 2^-7


def slack_case(oracle, dim, k=10, n=800):
    """The owner has half its features at UP and half at DOWN.  k "up" partners live on the first half with the value UP (times a
    power of two each: the same cosine bits, the same screening score): the screen sees them 0.0055 too high, and each lies in a span
    of its own, so that the k-th largest span maximum of the owner is their screening score.  One "down" partner lives on the second
    half with the value DOWN, and one small feature of the first half lifts its true cosine just above theirs, at about 0.71: it is
    the owner's best neighbour, and the screen sees it 0.0055 too low.  The gap of the screening scores is about 0.0097: more than m,
    less than 2 m.  A slack of m, or a conversion coarser than round-to-nearest-even, loses the owner's best neighbour."""
    rng = np.random.default_rng(300 + dim)
    h = dim // 2
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    sign = rng.choice([-1.0, 1.0], size=dim)
    owner = 70
    x = np.concatenate([np.full(h, UP), np.full(h, DOWN)]) * sign
    rows[owner] = x.astype(np.float32)
    ups = [32 * (2 * i + 1) + 3 + i for i in range(k)]  # blocks 1, 3, ..., 19: one span each
    for i, p in enumerate(ups):
        rows[p] = (np.concatenate([np.full(h, UP), np.zeros(h)]) * sign * 2.0 ** (i - 4)).astype(np.float32)
    down = 32 * 22 + 9
    q = np.concatenate([np.zeros(h), np.full(h, DOWN)])
    q[0] = DOWN * 2.0 ** -4
    rows[down] = (q * sign).astype(np.float32)
    rows = np.ascontiguousarray(rows)
    m = margin(dim)
    c_up = [oracle.canonical_score(rows[owner], rows[p]) for p in ups]
    c_down = oracle.canonical_score(rows[owner], rows[down])
    s_up = [screen_score(rows[owner], rows[p]) for p in ups]
    s_down = screen_score(rows[owner], rows[down])
    print("dim %d: c_up %.6f c_down %.6f s_up %.6f s_down %.6f gap %.5f m %.5f" % (dim, c_up[0], c_down, min(s_up), s_down, min(s_up) - s_down, m))
    assert len(set(c_up)) == 1 and 0.70 < c_up[0] < c_down < 0.72
    assert m < min(s_up) - s_down < 2 * m
    others = np.delete(np.arange(n), [owner, down] + ups)
    assert max(screen_score(rows[owner], rows[p]) for p in others) < s_down - 0.05  # nothing else is near
    return rows, owner, ups, down


@pytest.mark.parametrize("dim", [64, 384, 768])
def test_edge_of_the_slack(ctx, oracle, dim):
    k = 10
    rows, owner, ups, down = slack_case(oracle, dim, k)  # (asserts on the CPU before the device is used)
    ids = make_ids(np.random.default_rng(dim), rows.shape[0])
    s = build(ctx, rows, ids)
    got = s.neighbors(None, k)
    st = s.last_neighbor_stats()
    assert st["spans"] == 25 and st["sample_stride"] == 1  # every block a span: the k up partners are k span maxima
    check(got, reference(oracle, rows, ids, k))
    assert got[1][owner].tolist() == [ids[down]] + ids[ups[: k - 1]].tolist()
    s.close()


# ---- 4. tile-size boundaries ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,tile", [(64, 128), (576, 128), (640, 64), (1216, 64), (1280, 32)])
def test_tile_sizes(ctx, oracle, dim, tile):
    rng = np.random.default_rng(400 + dim)
    n, k = 800, 10
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    for r in (0, tile - 1, tile, n - 1):  # neighbours across the tile's edge and in the last, partial tile
        rows[(r + tile) % n] = neighbour(rng, rows[r], 0.95)
        rows[(r + 401) % n] = neighbour(rng, rows[r], 0.9)
    ids = make_ids(rng, n)
    want = reference(oracle, rows, ids, k)
    assert want[2][0, 0] > 0.94 and want[2][0, 1] > 0.85 and want[1][n - 1, 0] == ids[(n - 1 + tile) % n]
    s = build(ctx, rows, ids)
    got = s.neighbors(None, k)
    assert s.last_neighbor_stats()["tile_rows"] == tile
    check(got, want)
    s.close()


# ---- 5. ties -------------------------------------------------------------------------------------------------------------------
def test_ties(ctx, oracle):
    """Groups of 16 identical rows against k = 5 and 10: the cut falls inside the group, and position decides.  Then rows whose
    cosines with their owner differ in the last bits of the f64: one feature moved by one f32 ulp."""
    rng = np.random.default_rng(51)
    n = 600
    rows = rng.standard_normal((n, D)).astype(np.float32)
    groups = []
    for gi in range(3):
        members = np.sort(rng.permutation(n)[:16])
        rows[members] = rng.standard_normal(D).astype(np.float32)
        groups.append(members)
    taken = np.concatenate(groups)
    free = np.setdiff1d(np.arange(n), taken)
    owner, twins = int(free[0]), free[1:13]
    base = neighbour(rng, rows[owner], 0.9)
    for i, p in enumerate(twins):
        v = base.copy()
        v[i] = np.nextafter(v[i], np.float32(np.inf))
        rows[p] = v
    ids = make_ids(rng, n)
    c = np.array(sorted(oracle.canonical_score(rows[owner], rows[p]) for p in twins))
    gaps = np.diff(c)
    print("near ties: %d distinct of %d, largest gap %.3g" % (len(set(c.tolist())), len(c), gaps.max()))
    assert len(set(c.tolist())) >= 6 and gaps.max() < 1e-7
    s = build(ctx, rows, ids)
    for k in (5, 10):
        got = s.neighbors(None, k)
        check(got, reference(oracle, rows, ids, k))
        for members in groups:  # a member's list starts with the k lowest positions of the others
            for r in members[[0, 7, 15]]:
                others = members[members != r]
                assert got[1][r].tolist() == ids[others[:k]].tolist() and (got[2][r] > 0.9999).all()
    s.close()


# ---- 6. few rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 33])
def test_few_rows(ctx, oracle, n):
    rng = np.random.default_rng(60 + n)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids)
    for k in (1, 10, 64):
        got = s.neighbors(None, k)
        check(got, reference(oracle, rows, ids, k))
        assert (got[3] == min(k, n - 1)).all() and got[1].shape == (n, k)
    s.close()


# ---- 7. rows that take no part, wild rows --------------------------------------------------------------------------------------
def test_rows_that_take_no_part_and_wild_rows(ctx, oracle):
    rng = np.random.default_rng(71)
    n, k = 800, 10
    rows = rng.standard_normal((n, D)).astype(np.float32)
    rows[5] = 0.0
    # |x|^2 beside 2^-126: unit rows a little longer and a little shorter than 1, at 2^-63 of their length
    edge = list(range(200, 212))
    for i, r in enumerate(edge):
        u = rows[r].astype(np.float64)
        rows[r] = (u / np.linalg.norm(u) * (1.0 + (1e-3 if i % 2 else -1e-3)) * 2.0 ** -63).astype(np.float32)
    # wild rows: copies of rows 10.. at |x| about 2^-62 and 2^60 — true neighbours (cosine 1) the screen cannot certify
    wild = {300: (10, 2.0 ** -66), 301: (11, 2.0 ** 56), 500: (12, 2.0 ** -66), 501: (12, 2.0 ** 56)}
    for r, (src, sc) in wild.items():
        rows[r] = rows[src] * np.float32(sc)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    live = takes_part(rows)
    assert not live[5] and live[edge].sum() == 6 and (~live[edge]).sum() == 6 and live[list(wild)].all()
    n2 = (rows[list(wild)].astype(np.float64) ** 2).sum(axis=1)
    assert ((n2 < 2.0 ** -40) | (n2 > 2.0 ** 40)).all()
    s = build(ctx, rows, ids)
    got = s.neighbors(None, k)
    want = reference(oracle, rows, ids, k)
    check(got, want)
    assert (got[3][~live] == 0).all() and (got[1][~live] == -1).all() and not np.isin(got[1], ids[~live]).any()
    for r, (src, _sc) in wild.items():
        assert ids[r] in got[1][src, :2] and ids[src] in got[1][r, :2] and got[3][r] == k
    assert got[1][12, :2].tolist() == [ids[500], ids[501]]
    # hidden rows, a whole span among them (800 rows: every block is a span of its own)
    hidden = [20, 21, 150] + list(range(96, 128))
    s.hide_items(ids[hidden])
    part = np.ones(n, dtype=bool)
    part[hidden] = False
    h = s.neighbors(None, k)
    check(h, reference(oracle, rows, ids, k, part))
    assert (h[3][hidden] == 0).all() and len(h[0]) == n and not np.isin(h[1], ids[hidden]).any()
    s.unhide_items(ids[hidden])
    check(s.neighbors(None, k), want)
    # removed rows: n shrinks
    gone = [0, 33, 799]
    s.remove_items(ids[gone])
    keep = np.setdiff1d(np.arange(n), gone)
    r = s.neighbors(None, k)
    assert len(r[0]) == n - 3
    check(r, reference(oracle, rows[keep], ids[keep], k))
    s.close()


# ---- 8. segments, source lists, views ------------------------------------------------------------------------------------------
def test_segments_sources_and_views(ctx, oracle):
    rng = np.random.default_rng(81)
    sizes = [64, 96, 32, 1, 128, 5, 300]  # (a piece that is not the last of its source is a whole number of blocks: test_assign_gpu.py)
    src_of = [1, 2, 3, 1, 2, 3, 2]
    n, k = sum(sizes), 7
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    s = pa.Searcher(ctx, D, "cosine")
    first = np.concatenate([[0], np.cumsum(sizes)])
    where = {1: [], 2: [], 3: []}
    for i, sid in enumerate(src_of):
        s.reserve(sid, sizes[i])
        s.add_rows(sid, rows[first[i] : first[i + 1]], ids[first[i] : first[i + 1]])
        s.finalize()
        where[sid] += list(range(first[i], first[i + 1]))
    assert s.num_segments == 7 and s.num_rows == n

    def rows_of(sources):  # in global position order: by source, in the order the sources were created
        return np.array([r for sid in (1, 2, 3) if sid in sources for r in where[sid]], dtype=np.int64)

    for sources in (None, [1, 2, 3], [3, 1, 2], [2], [3, 1], [1]):
        sel = rows_of([1, 2, 3] if sources is None else sources)
        check(s.neighbors(sources, k), reference(oracle, rows[sel], ids[sel], k))
    empty = s.neighbors([], k)
    assert len(empty[0]) == 0 and empty[1].shape == (0, k) and empty[2].shape == (0, k) and len(empty[3]) == 0
    assert len(s.neighbors([99], k)[0]) == 0
    # a view equals a fresh searcher of its rows
    allowed = rows_of([1, 2, 3])[rng.random(n) < 0.4]
    v = s.view(ids[allowed])
    fresh = build(ctx, rows[allowed], ids[allowed])
    a, b = v.neighbors(None, k), fresh.neighbors(None, k)
    same(a, b)
    check(a, reference(oracle, rows[allowed], ids[allowed], k))
    assert v.last_neighbor_stats()["rows"] == len(allowed)
    v.close()
    fresh.close()
    # a source emptied by remove_items: its rows are gone from every list, and it selects nothing
    s.remove_items(ids[where[3]])
    assert len(s.neighbors([3], k)[0]) == 0
    sel = rows_of([1, 2])
    check(s.neighbors(None, k), reference(oracle, rows[sel], ids[sel], k))
    check(s.neighbors([2, 3], k), reference(oracle, rows[where[2]], ids[where[2]], k))
    s.close()


# ---- 9. list growth ------------------------------------------------------------------------------------------------------------
def test_list_growth(ctx, oracle):
    rng = np.random.default_rng(91)
    n, dim, k = 1024, 64, 10
    centre = rng.standard_normal(dim).astype(np.float32)
    rows = np.ascontiguousarray(np.stack([neighbour(rng, centre, 0.9995) for _ in range(n)]))
    ids = make_ids(rng, n)
    want = reference(oracle, rows, ids, k)
    # every pair is a candidate: the screening scores (exact arithmetic on the bf16 roundings; the f32 accumulation moves them by
    # 1e-5) all lie within 2 m - 0.001 of the largest one, and no threshold is above (largest screening score) - 2 m
    B = bf16_rne(rows).astype(np.float64)
    inv = 1.0 / np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1))
    S = (B @ B.T) * np.outer(inv, inv)
    off = ~np.eye(n, dtype=bool)
    print("screening scores %.5f .. %.5f" % (S[off].min(), S[off].max()))
    assert S[off].min() > S[off].max() - 2 * margin(dim) + 0.001
    s = build(ctx, rows, ids)
    got = s.neighbors(None, k)
    st = s.last_neighbor_stats()
    print(st)
    assert st["candidates"] == n * (n - 1) and st["candidates"] > max(65536, 32 * k * n) and st["reruns"] == 1
    check(got, want)
    s.close()


# ---- 10. independence of the search settings -----------------------------------------------------------------------------------
def test_independent_of_search_settings(ctx, oracle):
    rng = np.random.default_rng(101)
    n, k = 700, 10
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    want = reference(oracle, rows, ids, k)
    for copy, kernel, flags, cap in (("off", "auto", 0, None), ("int8", "auto", 32, 64), ("auto", "mfma", 0, 4096), ("auto", "wave", 32, None)):
        s = pa.Searcher(ctx, D, "cosine")
        s.set_screening_copy(copy)
        s.add_rows(1, rows, ids)
        s.finalize()
        s.set_kernel(kernel)
        s.set_tuning(flags)
        if cap:
            s.set_candidate_capacity(cap)
        check(s.neighbors(None, k), want)
        s.search_vectors(None, 5, rows[:3])  # a search in between leaves its pass state behind; the next call does not see it
        check(s.neighbors(None, k), want)
        s.close()


# ---- 11. the independent path: search by example -------------------------------------------------------------------------------
def test_equals_search_like(ctx):
    rng = np.random.default_rng(111)
    n, k = 3000, 10
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids)
    got = s.neighbors(None, k)
    assert len(set(ids.tolist())) == n and (got[3] == k).all()
    assert (np.diff(got[2].astype(np.float64), axis=1) < 0).all()  # no ties among the reported scores
    sample = np.sort(rng.permutation(n)[:256])
    l_ids, l_scores, l_counts, found = s.search_like(None, k, [[int(i)] for i in ids[sample]], exclude_examples=True)
    assert found.all() and (l_counts == k).all()
    np.testing.assert_array_equal(got[1][sample], l_ids)
    np.testing.assert_array_equal(bits(got[2][sample]), bits(l_scores))
    s.close()


# ---- 12. errors on the device --------------------------------------------------------------------------------------------------
def test_errors_on_the_device(ctx):
    wide = build(ctx, np.ones((40, 2560), dtype=np.float32), np.arange(40, dtype=np.int64))
    with pytest.raises(pa.PcvError) as e:
        wide.neighbors(None, 3)
    assert e.value.status == 3 and "neighbors" in str(e.value)  # PCV_ERR_UNSUPPORTED: rows wider than the self-join's tile
    wide.close()
    s = build(ctx, np.ones((40, D), dtype=np.float32), np.arange(40, dtype=np.int64))
    with pytest.raises(ValueError):
        s.neighbors(None, 65)
    s.add_rows(1, np.ones((1, D), dtype=np.float32), np.array([99], dtype=np.int64))  # pending rows: as a search
    with pytest.raises(pa.PcvError) as e:
        s.neighbors(None, 3)
    assert e.value.status == 1
    s.close()


# ---- 13. the C++ mirror --------------------------------------------------------------------------------------------------------
def test_cpp_mirror_neighbors_program():
    src = os.path.join(ROOT, "tests", "cpp", "neighbors_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "neighbors_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "neighbors_mirror_test: ok" in r.stdout
