"""GPU: item matches (pcv_searcher_match), through the Python mirror of the C ABI.  The reference of every check is match_ref.py: the
oracle's canonical cosine of every partner that can be among a row's k best, sorted (-c, position), cut at the score bound; ids,
counts and the f32 bits of the scores are compared for equality.  Each test first asserts on the CPU what makes its input hostile."""
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from duplicates_ref import bf16_rne, bits, build, make_ids, neighbour, screen_score
from match_ref import check, reference
from neighbors_ref import takes_part
from test_neighbors_gpu import margin, slack_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)


# ---- 1. the identity that defines the call -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("name", ["scan_n77_d100", "scan_n1000_d384"])
def test_square_is_neighbors(ctx, golden_dir, name, metric):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    rows = np.array(g["corpus"], dtype=np.float32)
    rng = np.random.default_rng(21)
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(rows.shape[0], 1))).astype(np.float32)
    rows = np.ascontiguousarray(rows)
    n = rows.shape[0]
    s = build(ctx, rows, make_ids(rng, n), metric)
    for k in (1, 10, 64):
        want = s.neighbors(None, k)
        nst = s.last_neighbor_stats()
        got = s.match(None, None, k)
        mst = s.last_match_stats()
        same(got, want)
        assert np.isnan(got[2][np.arange(k)[None, :] >= got[3][:, None]]).all()
        assert mst["candidates"] == nst["candidates"] and mst["listed"] == nst["listed"] and mst["rows"] == mst["partner_rows"] == n
        assert mst["owner_blocks"] == mst["partner_blocks"] == (n + 31) // 32 and mst["reruns"] == 0
        for f in ("k", "tile_rows", "sample_stride", "spans"):
            assert mst[f] == nst[f], f
        same(s.match([1], [1], k, -1.0), want)
    s.close()


# ---- 2. rectangles against the reference ---------------------------------------------------------------------------------------
SIZES = {"a": 300, "b": 500, "c": 200}
SID = {"a": 11, "b": 12, "c": 13}
SELECTIONS = [(["a"], ["b", "c"]), (["c"], ["a"]), (["a", "b"], ["b", "c"]), (["b"], ["b"]), (None, ["c"])]


def three_sources(dim):
    """1000 rows in the sources a, b, c (in that position order) with planted near rows across the sources, exact copies (ties), zero
    rows, hidden ids and an item id stored in two sources -> rows, ids, src (name per row), hidden ids"""
    rng = np.random.default_rng(200 + dim)
    n = sum(SIZES.values())
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    src = np.repeat(list(SIZES), list(SIZES.values()))
    for r, p, c in ((5, 310, 0.95), (5, 820, 0.9), (299, 300, 0.97), (420, 2, 0.93), (850, 17, 0.96), (850, 799, 0.92), (999, 0, 0.9)):
        rows[p] = neighbour(rng, rows[r], c)
    rows[640] = rows[100]                        # ties across the sources: 100 (a), 640 (b), 900 (c) are one direction
    rows[900] = rows[100] * np.float32(0.5)
    rows[[50, 333, 950]] = 0.0                   # no cosine
    ids = make_ids(rng, n)
    ids[700] = ids[40]                           # one item id in a and in b
    hidden = ids[[60, 61, 400, 960]]
    return np.ascontiguousarray(rows), ids, src, hidden


def masks(src, frm, to):
    every = list(SIZES)
    return np.isin(src, every if frm is None else frm), np.isin(src, every if to is None else to)


def sids(names):
    return None if names is None else [SID[x] for x in names]


@pytest.fixture(scope="module", params=[100, 384])
def rectangle(request, ctx):
    dim = request.param
    rows, ids, src, hidden = three_sources(dim)
    part = ~np.isin(ids, hidden)
    live = takes_part(rows, part)
    assert not live[[50, 333, 950, 60, 61, 400, 960]].any() and live.sum() == len(ids) - 7
    assert len(set(ids.tolist())) == len(ids) - 1 and src[40] == "a" and src[700] == "b"
    first = np.concatenate([[0], np.cumsum(list(SIZES.values()))])
    s = build(ctx, rows, ids, "cosine", [(SID[x], first[i], first[i + 1]) for i, x in enumerate(SIZES)])
    assert s.hide_items(hidden) == 4
    allowed = np.random.default_rng(dim).random(len(ids)) < 0.6
    allowed[[100, 640, 900, 40, 700]] = True
    v = s.view(ids[allowed])
    yield dict(s=s, v=v, rows=rows, ids=ids, src=src, part=part, allowed=allowed)
    v.close()
    s.close()


@pytest.mark.parametrize("through_view", [False, True])
@pytest.mark.parametrize("sel", range(len(SELECTIONS)))
def test_rectangles(oracle, rectangle, sel, through_view):
    frm, to = SELECTIONS[sel]
    r = rectangle
    if through_view:  # a view holds every row carrying an allowed id: the second row of the repeated id comes with the first
        keep = np.isin(r["ids"], r["ids"][r["allowed"]])
        rows, ids, src, part, s = r["rows"][keep], r["ids"][keep], r["src"][keep], r["part"][keep], r["v"]
    else:
        rows, ids, src, part, s = r["rows"], r["ids"], r["src"], r["part"], r["s"]
    owner, partner = masks(src, frm, to)
    for k in (1, 10):
        full = 0
        for lo in (-1.0, 0.2):
            want = reference(oracle, rows, ids, owner, partner, k, lo, part)
            if lo == -1.0:
                full = int(want[3].sum())
            else:  # what is hostile: the bound leaves matches and (k = 10: in every case) takes some away
                assert 0 < want[3].sum() <= full and (k == 1 or want[3].sum() < full)
            got = s.match(sids(frm), sids(to), k, lo)
            check(got, want)
            st = s.last_match_stats()
            assert st["rows"] == owner.sum() and st["partner_rows"] == partner.sum() and st["listed"] == want[3].sum()
            assert st["candidates"] >= st["listed"] and st["k"] == k


def test_rectangle_ties_and_order_of_the_selection(oracle, rectangle):
    """100 (a), 640 (b) and 900 (c) point one way: wherever two of them are partners of one owner, the lower position comes first,
    also where the launch order ([to only | to and from | from only]) is not the position order.  A list of sources is a set."""
    r = rectangle
    s, ids = r["s"], r["ids"]
    got = s.match(sids(["a", "b"]), sids(["b", "c"]), 3)
    assert got[1][100, :2].tolist() == [ids[640], ids[900]] and got[1][640, 0] == ids[900]
    got = s.match(sids(["b", "c"]), sids(["a", "b"]), 3)  # launch order a, b, c: a is `to` only
    assert got[1][640 - 300, 0] == ids[100] and got[1][900 - 300, :2].tolist() == [ids[100], ids[640]]
    got = s.match(sids(["a", "b"]), sids(["a", "c"]), 3)  # launch order c, a, b: the partner stored last is streamed first
    assert got[1][640, :2].tolist() == [ids[100], ids[900]] and got[1][100, 0] == ids[900]
    got = s.match(sids(["c"]), sids(["a", "b"]), 3)
    assert got[1][900 - 800, :2].tolist() == [ids[100], ids[640]]
    same(s.match(sids(["b", "a"]), sids(["c", "b"]), 5, 0.1), s.match(sids(["a", "b"]), sids(["b", "c"]), 5, 0.1))
    # the item id stored in a and in b: each of the two rows is a partner like any other, the other one included
    owner, partner = masks(r["src"], ["a"], ["b"])
    want = reference(oracle, r["rows"], ids, owner, partner, 64, -1.0, r["part"])
    got = s.match(sids(["a"]), sids(["b"]), 64)
    check(got, want)
    assert got[0][40] == ids[700]


# ---- 3. the independent path: search -------------------------------------------------------------------------------------------
def test_equals_search(ctx):
    rng = np.random.default_rng(31)
    dim, k = 384, 10
    a, b = 200, 2500
    rows = rng.standard_normal((a + b, dim)).astype(np.float32)
    ids = make_ids(rng, a + b)
    U = rows.astype(np.float64)
    U /= np.linalg.norm(U, axis=1)[:, None]
    top = -np.sort(-(U[:a] @ U[a:].T), axis=1)[:, : k + 1]
    assert (np.diff(top, axis=1) < -1e-9).all()  # no two of a row's top k + 1 cosines tie (f64 by numpy: D * 2^-53 from the canonical one)
    s = build(ctx, rows, ids, "cosine", [(1, 0, a), (2, a, a + b)])
    got = s.match([1], [2], k)
    assert (got[3] == k).all()
    s_ids, s_scores, s_counts = s.search_vectors([2], k, rows[:a])
    assert (np.asarray(s_counts) == k).all()
    np.testing.assert_array_equal(got[0], ids[:a])
    np.testing.assert_array_equal(got[1], s_ids)
    np.testing.assert_array_equal(bits(got[2]), bits(s_scores))
    s.close()


# ---- 4. the edge of the score bound --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 384])
def test_edge_of_the_score_bound(ctx, oracle, dim):
    """slack_case of test_neighbors_gpu.py: the `down` partner's c is the bound itself or just above it and the bf16 screen sees it
    0.0055 too low; the k `up` partners' c is just below the bound and the screen sees them 0.0055 too high.  A screen that decided
    the bound alone — or a threshold of min_score without the margin — would list the ups and lose the down."""
    k = 10
    rows, owner, ups, down = slack_case(oracle, dim, k)
    rng = np.random.default_rng(dim)
    to_rows = rows.copy()
    x = rows[owner].copy()
    to_rows[owner] = rng.standard_normal(dim).astype(np.float32)  # the owner lives in `from` alone
    from_rows = rng.standard_normal((40, dim)).astype(np.float32)
    from_rows[33] = x
    c_down = oracle.canonical_score(x, rows[down])
    c_up = oracle.canonical_score(x, rows[ups[0]])
    lo = np.float32(c_down)
    if float(lo) > c_down:
        lo = np.nextafter(lo, np.float32(-1.0))
    m = margin(dim)
    s_down, s_up = screen_score(x, rows[down]), screen_score(x, rows[ups[0]])
    print("dim %d: bound %.9g c_down %.9g c_up %.9g s_down %.6f s_up %.6f m %.5f" % (dim, float(lo), c_down, c_up, s_down, s_up, m))
    assert c_up < float(lo) <= c_down and c_down - float(lo) < 1e-7
    assert float(lo) - m < s_down < float(lo) - 0.005  # seen too low, by less than the margin
    assert s_up - c_up > 0.005 and s_up > float(lo) + 0.004  # seen 0.0055 too high: well above the bound its c is below
    assert max(oracle.canonical_score(x, to_rows[p]) for p in range(len(to_rows)) if p != down and p not in ups) < float(lo) - 0.05
    allr = np.ascontiguousarray(np.concatenate([to_rows, from_rows]))
    nt = len(to_rows)
    ids = make_ids(rng, len(allr))
    s = build(ctx, allr, ids, "cosine", [(1, 0, nt), (2, nt, len(allr))])
    owner_m, partner_m = np.arange(len(allr)) >= nt, np.arange(len(allr)) < nt
    got = s.match([2], [1], k, float(lo))
    st = s.last_match_stats()
    assert st["spans"] == 25 and st["sample_stride"] == 1  # every partner block a span: the k ups are k span maxima above the down
    check(got, reference(oracle, allr, ids, owner_m, partner_m, k, float(lo)))
    assert got[3][33] == 1 and got[1][33].tolist() == [ids[down]] + [-1] * (k - 1) and np.isnan(got[2][33, 1:]).all()
    assert bits(got[2][33, :1])[0] == bits(np.float32(c_down))[()]
    # one f32 step up, the bound is above c_down: the down goes too
    hi = np.nextafter(lo, np.float32(1.0))
    assert float(hi) > c_down
    got = s.match([2], [1], k, float(hi))
    assert got[3][33] == 0 and (got[1][33] == -1).all() and np.isnan(got[2][33]).all()
    # and without a bound the ups come back behind it
    got = s.match([2], [1], k)
    assert got[1][33].tolist() == [ids[down]] + ids[ups[: k - 1]].tolist()
    s.close()


# ---- 5. the sampled bound pass looks at partner blocks only --------------------------------------------------------------------
@pytest.mark.parametrize("from_first", [False, True])
def test_sampled_bound_pass_over_the_partners_only(ctx, oracle, from_first):
    """`to`: 12 320 rows of 64 features, 385 blocks of which every fourth is sampled.  `from`: 100 rows of a source of their own, stored
    before `to` or behind it.  The owners 0..49 have two 0.999-partners each in `to` blocks the sample skips (block numbers 1 and 3
    modulo 4); the owners 50..99 are 0.9999-copies of them — decoys inside `from`, nobody's partner."""
    rng = np.random.default_rng(52)
    nt, nf, dim, k = 12320, 100, 64, 10
    to_rows = rng.standard_normal((nt, dim)).astype(np.float32)
    from_rows = rng.standard_normal((nf, dim)).astype(np.float32)
    planted = {}
    for i in range(50):
        spots = [(4 * i + 1) * 32 + (i % 32), (4 * (i + 40) + 3) * 32 + (7 * i % 32)]
        for p in spots:
            to_rows[p] = neighbour(rng, from_rows[i], 0.999) * np.float32(rng.uniform(0.5, 2.0))
        from_rows[50 + i] = neighbour(rng, from_rows[i], 0.9999)
        planted[i] = spots
    assert all((p // 32) % 4 in (1, 3) and p < nt for spots in planted.values() for p in spots)
    assert len({p for spots in planted.values() for p in spots}) == 100
    if from_first:
        rows, f0, t0 = np.concatenate([from_rows, to_rows]), 0, nf
        layout = [(1, 0, nf), (2, nf, nf + nt)]
    else:
        rows, f0, t0 = np.concatenate([to_rows, from_rows]), nt, 0
        layout = [(2, 0, nt), (1, nt, nt + nf)]
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, nt + nf)
    pos = np.arange(nt + nf)
    owner, partner = (pos >= f0) & (pos < f0 + nf), (pos >= t0) & (pos < t0 + nt)
    want = reference(oracle, rows, ids, owner, partner, k)
    for i, spots in planted.items():  # what is hostile: the planted rows are the best two of the owner and of its decoy, far above the rest
        for o in (i, 50 + i):
            assert set(want[1][o, :2].tolist()) == set(ids[[t0 + p for p in spots]].tolist()), o
            assert want[2][o, 1] > 0.99 and want[2][o, 2] < 0.7
        assert oracle.canonical_score(from_rows[i], from_rows[50 + i]) > 0.9998  # the decoy would be the best partner, were it one
    s = build(ctx, rows, ids, "cosine", layout)
    got = s.match([1], [2], k)
    st = s.last_match_stats()
    print(st)
    assert st["sample_stride"] > 1 and st["spans"] > k and st["tile_rows"] == 128 and st["rows"] == nf and st["partner_rows"] == nt
    assert st["owner_blocks"] == 4 and st["partner_blocks"] == 385
    check(got, want)
    assert not np.isin(got[1], ids[owner]).any()  # no decoy, no row of `from` at all
    s.close()


# ---- 6. fewer partners than k --------------------------------------------------------------------------------------------------
def test_fewer_partners_than_k(ctx, oracle):
    rng = np.random.default_rng(61)
    dim, k = 384, 10
    rows = rng.standard_normal((47, dim)).astype(np.float32)  # source 1: 40 rows; source 2: 7 rows, 5 of them participating
    rows[42] = 0.0
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, 47)
    s = build(ctx, rows, ids, "cosine", [(1, 0, 40), (2, 40, 47)])
    assert s.hide_items(ids[[45]]) == 1
    part = np.ones(47, dtype=bool)
    part[45] = False
    pos = np.arange(47)
    assert (takes_part(rows, part) & (pos >= 40)).sum() == 5
    got = s.match(None, [2], k)
    check(got, reference(oracle, rows, ids, None, pos >= 40, k, -1.0, part))
    assert (got[3][:40] == 5).all() and got[3][40:].tolist() == [4, 4, 0, 4, 4, 0, 4]
    assert (got[1][:, 5:] == -1).all() and np.isnan(got[2][:, 5:]).all()
    st = s.last_match_stats()
    assert st["rows"] == 47 and st["partner_rows"] == 7 and st["listed"] == 40 * 5 + 5 * 4 and st["owner_blocks"] == 3 and st["partner_blocks"] == 1
    for to in ([], [99]):  # `to` selects nothing: n is still reported, with every id
        e = s.match([1], to, k)
        np.testing.assert_array_equal(e[0], ids[:40])
        assert (e[3] == 0).all() and (e[1] == -1).all() and np.isnan(e[2]).all() and e[1].shape == (40, k)
        st = s.last_match_stats()
        assert st["rows"] == 40 and st["partner_rows"] == 0 and st["partner_blocks"] == 0 and st["candidates"] == 0 and st["listed"] == 0
    for frm in ([], [99]):
        e = s.match(frm, None, k)
        assert len(e[0]) == 0 and e[1].shape == (0, k) and e[2].shape == (0, k) and len(e[3]) == 0
    s.close()


# ---- 7. the work is |from| x |to| ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("from_first", [False, True])
def test_work_is_proportional_to_the_rectangle(ctx, oracle, from_first):
    """40 owners against 9 600 partners: two owner blocks, 300 partner blocks.  The owners are 40 of the union's 9 640 rows and a
    row's candidates are as many in both calls up to the sample's luck, so `neighbors` over the union lists about 241 times the
    candidates; the test asks for 50 times, which leaves that luck a factor of almost five."""
    rng = np.random.default_rng(72)
    nf, nt, dim, k = 40, 9600, 64, 10
    rows = np.ascontiguousarray(rng.standard_normal((nf + nt, dim)).astype(np.float32))
    ids = make_ids(rng, nf + nt)
    pos = np.arange(nf + nt)
    if from_first:
        layout, owner = [(1, 0, nf), (2, nf, nf + nt)], pos < nf
    else:
        layout, owner = [(2, 0, nt), (1, nt, nt + nf)], pos >= nt
    s = build(ctx, rows, ids, "cosine", layout)
    got = s.match([1], [2], k)
    st = s.last_match_stats()
    print(st)
    assert st["owner_blocks"] == 2 and st["partner_blocks"] == 300 and st["rows"] == nf and st["partner_rows"] == nt
    check(got, reference(oracle, rows, ids, owner, ~owner, k))
    assert st["listed"] == nf * k and st["candidates"] >= st["listed"]
    s.neighbors(None, k)
    union = s.last_neighbor_stats()
    print(union)
    assert union["candidates"] > 50 * st["candidates"]
    s.close()


# ---- 8. list growth ------------------------------------------------------------------------------------------------------------
def test_list_growth(ctx, oracle):
    rng = np.random.default_rng(81)
    nf, nt, dim, k = 64, 2048, 64, 10
    centre = rng.standard_normal(dim).astype(np.float32)
    rows = np.ascontiguousarray(np.stack([neighbour(rng, centre, 0.9995) for _ in range(nt + nf)]))
    ids = make_ids(rng, nt + nf)
    pos = np.arange(nt + nf)
    # every (owner, partner) pair is a candidate: the screening scores (exact arithmetic on the bf16 roundings; the f32 accumulation
    # moves them by 1e-5) all lie within 2 m - 0.001 of the largest one, and no threshold is above (largest screening score) - 2 m
    B = bf16_rne(rows).astype(np.float64)
    inv = 1.0 / np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1))
    S = ((B[nt:] @ B[:nt].T) * np.outer(inv[nt:], inv[:nt]))
    print("screening scores %.5f .. %.5f" % (S.min(), S.max()))
    assert S.min() > S.max() - 2 * margin(dim) + 0.001
    assert nf * nt > max(65536, 32 * k * nf)  # more than the first list holds
    s = build(ctx, rows, ids, "cosine", [(2, 0, nt), (1, nt, nt + nf)])
    got = s.match([1], [2], k)
    st = s.last_match_stats()
    print(st)
    assert st["candidates"] == nf * nt and st["reruns"] == 1
    check(got, reference(oracle, rows, ids, pos >= nt, pos < nt, k))
    s.close()


# ---- 9. independence of the search settings, errors on the device ---------------------------------------------------------------
def test_independent_of_search_settings(ctx, oracle):
    rng = np.random.default_rng(91)
    n, dim, k = 700, 384, 10
    rows = np.ascontiguousarray(rng.standard_normal((n, dim)).astype(np.float32))
    ids = make_ids(rng, n)
    pos = np.arange(n)
    want = reference(oracle, rows, ids, pos < 200, pos >= 100, k, 0.05)
    for copy, kernel, flags, cap in (("off", "auto", 0, None), ("int8", "auto", 32, 64), ("auto", "mfma", 0, 4096), ("auto", "wave", 32, None)):
        s = pa.Searcher(ctx, dim, "cosine")
        s.set_screening_copy(copy)
        for sid, lo, hi in ((1, 0, 100), (2, 100, 200), (3, 200, n)):
            s.add_rows(sid, rows[lo:hi], ids[lo:hi])
        s.finalize()
        s.set_kernel(kernel)
        s.set_tuning(flags)
        if cap:
            s.set_candidate_capacity(cap)
        check(s.match([1, 2], [2, 3], k, 0.05), want)
        s.search_vectors(None, 5, rows[:3])  # a search in between leaves its pass state behind; the next call does not see it
        check(s.match([1, 2], [2, 3], k, 0.05), want)
        s.close()


def test_errors_on_the_device(ctx):
    wide = build(ctx, np.ones((40, 2560), dtype=np.float32), np.arange(40, dtype=np.int64))
    with pytest.raises(pa.PcvError) as e:
        wide.match(None, None, 3)
    assert e.value.status == 3 and "match" in str(e.value)  # PCV_ERR_UNSUPPORTED: rows wider than the screen's tile
    wide.close()
    s = build(ctx, np.ones((40, 384), dtype=np.float32), np.arange(40, dtype=np.int64))
    with pytest.raises(ValueError):
        s.match(None, None, 65)
    with pytest.raises(pa.PcvError) as e:
        s.match(None, None, 3, 1.5)
    assert e.value.status == 1
    s.add_rows(1, np.ones((1, 384), dtype=np.float32), np.array([99], dtype=np.int64))  # pending rows: as a search
    with pytest.raises(pa.PcvError) as e:
        s.match(None, None, 3)
    assert e.value.status == 1
    s.close()


# ---- 10. the C++ mirror --------------------------------------------------------------------------------------------------------
def test_cpp_mirror_match_program():
    src = os.path.join(ROOT, "tests", "cpp", "match_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "match_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match_mirror_test: ok" in r.stdout
