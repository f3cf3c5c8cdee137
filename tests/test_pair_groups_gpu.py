"""GPU: the group-aware pair calls (pcv_searcher_neighbors_grouped, _match_grouped, _find_duplicates_grouped), through the Python
mirror of the C ABI.  The reference of every check is pair_groups_ref.py; ids, counts, partner groups and the f32 bits of the scores are
compared for equality.  Each test first asserts on the CPU what makes its input hostile."""
import os
import subprocess

import numpy as np
import pytest

import duplicates_ref
import pair_groups_ref as ref
import perceive_amd as pa
from duplicates_ref import bf16_rne, bits, build, make_ids, neighbour
from neighbors_ref import takes_part

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384
SKIP, ONE = ref.SKIP_OWN, ref.ONE_PER_GROUP


def margin(dim):
    """selfjoin_margin at the padded dimension (selfjoin_kernels.hip)"""
    dp = (dim + 63) // 64 * 64
    return 0.00783 + 1.02 * ((dp + 16) * 1.2e-7) + 1e-6


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)


def plain_of(g):
    """(ids, partner ids, scores, counts) of a grouped result: the shape of the plain call's"""
    return g[0], g[1], g[2], g[4]


def set_row_groups(s, ids, groups):
    """the table that gives row i the group groups[i] (ids distinct, or equal ids with equal groups)"""
    s.clear_groups()
    has = groups >= 0
    if has.any():
        s.set_groups(ids[has], groups[has])


def screen_scores(owner, rows):
    """the screen's score of `owner` with every row, in exact arithmetic on the bf16 roundings (duplicates_ref.screen_score, vectorised)"""
    inv = 1.0 / np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1))
    inv_o = 1.0 / np.sqrt((owner.astype(np.float64) ** 2).sum())
    return (bf16_rne(rows).astype(np.float64) @ bf16_rne(owner).astype(np.float64)) * inv * inv_o


def golden(golden_dir, name, metric, seed=21):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    rows = np.array(g["corpus"], dtype=np.float32)
    rng = np.random.default_rng(seed)
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(rows.shape[0], 1))).astype(np.float32)
    return np.ascontiguousarray(rows), make_ids(rng, rows.shape[0])


# ---- 1. identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scan_n77_d100", "scan_n1000_d384"])
def test_identities(ctx, golden_dir, name):
    rows, ids = golden(golden_dir, name, "cosine")
    n = rows.shape[0]
    s = build(ctx, rows, ids, sources=[(1, 0, n // 2), (2, n // 2, n)])
    dup = s.find_duplicates(None, 0.3)
    dup_c = s.last_duplicate_stats()["candidates"]
    assert len(dup[0]) > 0

    def every_flag_is_plain(flag_list, groups_want):
        for k in (1, 10):
            want = s.neighbors(None, k)
            want_c = s.last_neighbor_stats()["candidates"]
            mwant = s.match([1], [2], k, 0.05)
            mwant_c = s.last_match_stats()["candidates"]
            for flags in flag_list:
                got = s.neighbors_grouped(None, k, flags)
                same(plain_of(got), want)
                assert s.last_neighbor_stats()["candidates"] == want_c and s.last_pair_group_stats()["flags"] == flags
                groups_want(got)
                mgot = s.match_grouped([1], [2], k, 0.05, flags)
                same(plain_of(mgot), mwant)
                assert s.last_match_stats()["candidates"] == mwant_c
                groups_want(mgot)
        gd = s.find_duplicates_grouped(None, 0.3)
        same(gd[:3], dup[:3])
        assert gd[3] == dup[3] and gd[4] == 0 and s.last_duplicate_stats()["candidates"] == dup_c

    def no_groups(got):
        assert (got[3] == -1).all()

    # (b) no table at all, every flag: the grouped kernels against the plain ones
    every_flag_is_plain((0, 1, 2, 3), no_groups)
    assert s.last_pair_group_stats()["grouped_rows"] == 0
    # (c) every id mapped to PCV_NO_GROUP
    s.set_groups(ids, np.full(n, -1, dtype=np.int64))
    assert s.group_stats()["entries"] == n
    every_flag_is_plain((0, 1, 2, 3), no_groups)
    s.clear_groups()
    every_flag_is_plain((3,), no_groups)
    # (a) flags == 0 with a table: the plain call, with the partners' groups beside it
    s.set_groups(ids, ids // 8)

    def id_groups(got):
        used = got[1] >= 0
        np.testing.assert_array_equal(got[3][used], got[1][used] // 8)
        assert (got[3][~used] == -1).all()

    for k in (1, 10, 64):
        want = s.neighbors(None, k)
        want_c = s.last_neighbor_stats()["candidates"]
        got = s.neighbors_grouped(None, k, 0)
        same(plain_of(got), want)
        assert s.last_neighbor_stats()["candidates"] == want_c
        id_groups(got)
        mwant = s.match([2], [1, 2], k, -1.0)
        mgot = s.match_grouped([2], [1, 2], k, -1.0, 0)
        same(plain_of(mgot), mwant)
        id_groups(mgot)
    st = s.last_pair_group_stats()
    assert st["flags"] == 0 and st["grouped_rows"] == int(takes_part(rows).sum()) and st["sibling_candidates"] == 0 and st["collapsed"] == 0
    s.close()


# ---- 2. golden corpora against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("name", ["scan_n77_d100", "scan_n1000_d384"])
def test_golden(ctx, oracle, golden_dir, name, metric):
    rows, ids = golden(golden_dir, name, metric)
    n = rows.shape[0]
    live = takes_part(rows)
    s = build(ctx, rows, ids, metric)
    for groups in (ids // 8, ids % 7):
        sizes = np.bincount(groups[live])
        assert sizes.max() >= 2  # siblings exist
        set_row_groups(s, ids, groups)
        for flags in (1, 2, 3):
            for k in (1, 10, 64):
                got = s.neighbors_grouped(None, k, flags)
                ref.check(got, ref.reference(oracle, rows, ids, groups, k, flags))
                st = s.last_pair_group_stats()
                assert st["flags"] == flags and st["grouped_rows"] == int(live.sum()) and st["bound_tile_rows"] <= 64
                assert st["collapsed"] == 0 or flags & ONE
                assert s.last_neighbor_stats()["k"] == k and s.last_neighbor_stats()["listed"] == int(got[4].sum())
    s.close()


# ---- 3, 4. the bound pass at 12 320 x 64 ------------------------------------------------------------------------------------------
N3, DIM3, K3 = 12320, 64, 10  # 385 blocks: every fourth is sampled (97), spans of two sampled blocks: 49 spans


def span_of(pos):
    """the span of a row in a SAMPLED block (a multiple of 4), -1 for a row the bound pass does not stream"""
    blk = pos // 32
    return np.where(blk % 4 == 0, blk // 8, -1)


def span_maxima(scores, skip):
    """per span the largest screening score over its sampled rows (`skip`: rows left out) and the row reaching it"""
    sp = span_of(np.arange(scores.size))
    best, arg = np.full(49, -np.inf), np.full(49, -1)
    for r in np.nonzero((sp >= 0) & ~skip)[0]:
        if scores[r] > best[sp[r]]:
            best[sp[r]], arg[sp[r]] = scores[r], r
    return best, arg


def test_bound_pass_leaves_the_owners_siblings_out(ctx, oracle):
    """The owner has 16 siblings at cosine 0.9999, one in a sampled block of each of 16 spans; nothing else is above 0.6.  Span maxima
    that count the siblings put the threshold near 0.98: no true neighbour is listed, and no filter behind the screen brings one back."""
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((N3, DIM3)).astype(np.float32)
    owner = 5000
    sib = [8 * 32 * s_ + 3 + s_ for s_ in range(2, 18)]  # block 8 s: sampled, span s
    for p in sib:
        rows[p] = neighbour(rng, rows[owner], 0.9999) * np.float32(rng.uniform(0.5, 2.0))
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, N3)
    groups = (np.arange(N3) // 8 + 100).astype(np.int64)  # documents of eight consecutive rows
    groups[[owner] + sib] = 7
    m = margin(DIM3)
    sc = screen_scores(rows[owner], rows)
    sc[owner] = -np.inf
    mine = groups == 7
    assert len(set(span_of(np.array(sib)).tolist())) == 16 and (span_of(np.array(sib)) >= 0).all()
    with_sib, _ = span_maxima(sc, np.arange(N3) == owner)
    tenth = np.sort(with_sib)[-K3]
    assert sc[~mine].max() <= 0.6 and tenth - 2 * m - 1e-4 > 0.6 + m  # (1e-4: the f32 accumulation beside the exact model)
    without, _ = span_maxima(sc, mine)
    assert np.sort(without)[-K3] < 0.6
    own = np.zeros(N3, dtype=bool)
    own[[owner, 0, 77, N3 - 1] + sib[:3]] = True
    want = ref.reference(oracle, rows, ids, groups, K3, SKIP, owner=own)
    at = int(np.cumsum(own)[owner] - 1)
    assert want[4][at] == K3 and want[2][at, 0] < 0.61 and not np.isin(want[1][at], ids[mine]).any()
    s = build(ctx, rows, ids)
    set_row_groups(s, ids, groups)
    got = s.neighbors_grouped(None, K3, SKIP)
    st, gst = s.last_neighbor_stats(), s.last_pair_group_stats()
    print(st, gst)
    assert st["sample_stride"] == 4 and st["spans"] == 49 and gst["bound_tile_rows"] == 64 and gst["grouped_rows"] == N3
    ref.check(tuple(x[own] for x in got), want)
    assert got[4][owner] == K3
    # the plain call is what the siblings fill
    assert np.isin(s.neighbors(None, K3)[1][owner], ids[sib]).all()
    s.close()


def test_threshold_counts_groups_not_partners(ctx, oracle):
    """One foreign group of 600 rows at cosine 0.99 of the owner has a member in a sampled block of every span: the ten largest span
    maxima are ten partners of ONE group.  A threshold from the tenth of them lists that group alone."""
    rng = np.random.default_rng(4)
    rows = rng.standard_normal((N3, DIM3)).astype(np.float32)
    owner = 7001
    big = [8 * 32 * s_ + j for s_ in range(49) for j in range(12)] + [4 * 32 + j for j in range(12)]
    assert len(big) == 600 and owner not in big
    for p in big:
        rows[p] = neighbour(rng, rows[owner], 0.99) * np.float32(rng.uniform(0.5, 2.0))
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, N3)
    groups = (np.arange(N3) // 8 + 100).astype(np.int64)
    groups[big] = 5
    own_sibs = [owner + 1, owner + 2, 40]
    groups[[owner] + own_sibs] = 6
    m = margin(DIM3)
    sc = screen_scores(rows[owner], rows)
    sc[owner] = -np.inf
    best, arg = span_maxima(sc, np.arange(N3) == owner)
    top = np.argsort(-best)[:K3]
    assert (groups[arg[top]] == 5).all()  # the ten largest span maxima carry one tag
    assert best[top].min() - 2 * m - 1e-4 > 0.6 + m and sc[groups != 5].max() <= 0.6  # a partner-counting threshold lists only the big group
    own = np.zeros(N3, dtype=bool)
    own[[owner, 0, big[0], big[599], N3 - 1]] = True
    at = int(np.cumsum(own)[owner] - 1)
    s = build(ctx, rows, ids)
    set_row_groups(s, ids, groups)
    for flags in (ONE, SKIP | ONE):
        want = ref.reference(oracle, rows, ids, groups, K3, flags, owner=own)
        assert want[4][at] == K3 and want[3][at, 0] == 5 and (want[3][at, 1:] != 5).all() and want[2][at, 1] < 0.61
        assert len(set(want[3][at].tolist())) == K3 and (flags == ONE or not (want[3][at] == 6).any())
        got = s.neighbors_grouped(None, K3, flags)
        ref.check(tuple(x[own] for x in got), want)
        assert s.last_pair_group_stats()["collapsed"] >= 599
    s.close()


# ---- 5. tag collision ------------------------------------------------------------------------------------------------------------
def test_colliding_tags_do_not_reach_the_exact_steps(ctx, oracle):
    rng = np.random.default_rng(5)
    n, dim, k = 300, 64, 10
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    g, h = 12345, 12345 + 2 ** 31
    assert ((g & 0x7FFFFFFF) + 1) == ((h & 0x7FFFFFFF) + 1)  # one tag
    owner, best, other, sib = 100, 200, 201, 101
    rows[best] = neighbour(rng, rows[owner], 0.95)
    rows[other] = neighbour(rng, rows[owner], 0.9)
    rows[sib] = neighbour(rng, rows[owner], 0.99)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    groups = np.full(n, -1, dtype=np.int64)
    groups[::3] = np.arange(0, n, 3) // 9
    s = build(ctx, rows, ids)
    # flags 1: the owner in g, its true best partner in g + 2^31
    groups[[owner, sib]] = g
    groups[best] = h
    set_row_groups(s, ids, groups)
    want = ref.reference(oracle, rows, ids, groups, k, SKIP)
    assert want[1][owner, 0] == ids[best] and want[3][owner, 0] == h and ids[sib] not in want[1][owner]
    ref.check(s.neighbors_grouped(None, k, SKIP), want)
    # flags 2: two partners in the two colliding groups are both kept
    groups[[owner, sib]] = -1
    groups[other] = g
    set_row_groups(s, ids, groups)
    want = ref.reference(oracle, rows, ids, groups, k, ONE)
    assert want[1][owner, :3].tolist() == [ids[sib], ids[best], ids[other]] and want[3][owner, 1:3].tolist() == [h, g]
    ref.check(s.neighbors_grouped(None, k, ONE), want)
    ref.check(s.neighbors_grouped(None, k, SKIP | ONE), ref.reference(oracle, rows, ids, groups, k, SKIP | ONE))
    s.close()


# ---- 6. short rows ---------------------------------------------------------------------------------------------------------------
def test_fewer_groups_than_k(ctx, oracle):
    rng = np.random.default_rng(6)
    n, k = 300, 10
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    groups = (np.arange(n) % 3).astype(np.int64)
    s = build(ctx, rows, ids)
    set_row_groups(s, ids, groups)
    for flags, count in ((ONE, 3), (SKIP | ONE, 2)):
        got = s.neighbors_grouped(None, k, flags)
        ref.check(got, ref.reference(oracle, rows, ids, groups, k, flags))
        assert (got[4] == count).all()  # fewer than k groups: no threshold, every partner is listed
        assert s.last_neighbor_stats()["candidates"] == n * (n - 1)
    s.close()


@pytest.mark.parametrize("n", [1, 2, 33])
def test_few_rows(ctx, oracle, n):
    rng = np.random.default_rng(60 + n)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    groups = (np.arange(n) % 4).astype(np.int64)
    groups[n // 2] = -1
    s = build(ctx, rows, ids)
    set_row_groups(s, ids, groups)
    for flags in (1, 2, 3):
        for k in (1, 10, 64):
            got = s.neighbors_grouped(None, k, flags)
            ref.check(got, ref.reference(oracle, rows, ids, groups, k, flags))
            assert got[1].shape == (n, k) and got[3].shape == (n, k)
    s.close()


# ---- 7. tile boundaries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,tile", [(576, 128), (640, 64), (1216, 64), (1280, 32)])
def test_tile_sizes(ctx, oracle, dim, tile):
    rng = np.random.default_rng(700 + dim)
    n, k = 800, 10
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    for r in (0, tile - 1, tile, n - 1):  # neighbours across the tile's edge and in the last, partial tile: siblings and foreign rows
        rows[(r + tile) % n] = neighbour(rng, rows[r], 0.95)
        rows[(r + 401) % n] = neighbour(rng, rows[r], 0.9)
        rows[(r + 402) % n] = neighbour(rng, rows[r], 0.85)
    ids = make_ids(rng, n)
    groups = (np.arange(n) % 100).astype(np.int64)  # r, r + tile (where tile % 100 != 0) ... r + 400 is a sibling of r
    groups[[tile % n, (2 * tile) % n]] = groups[0]
    want = ref.reference(oracle, rows, ids, groups, k, SKIP | ONE)
    assert want[2][0, 0] > 0.8 and len(set(want[3][0].tolist())) == k
    s = build(ctx, rows, ids)
    set_row_groups(s, ids, groups)
    got = s.neighbors_grouped(None, k, SKIP | ONE)
    assert s.last_neighbor_stats()["tile_rows"] == tile and s.last_pair_group_stats()["bound_tile_rows"] == min(tile, 64)
    ref.check(got, want)
    s.close()


# ---- 8. searcher state -----------------------------------------------------------------------------------------------------------
def test_searcher_state(ctx, oracle):
    rng = np.random.default_rng(81)
    sizes = [64, 96, 32, 1, 128, 5, 300]
    src_of = [1, 2, 3, 1, 2, 3, 2]
    n, k = sum(sizes), 7
    rows = rng.standard_normal((n, D)).astype(np.float32)
    rows[17] = 0.0
    ids = make_ids(rng, n)
    s = pa.Searcher(ctx, D, "cosine")
    first = np.concatenate([[0], np.cumsum(sizes)])
    where = {1: [], 2: [], 3: []}
    for i, sid in enumerate(src_of):
        s.reserve(sid, sizes[i])
        s.add_rows(sid, rows[first[i] : first[i + 1]], ids[first[i] : first[i + 1]])
        s.finalize()
        where[sid] += list(range(first[i], first[i + 1]))
    assert s.num_segments == 7
    order = np.array([r for sid in (1, 2, 3) for r in where[sid]], dtype=np.int64)  # global position order
    R, I = rows[order], ids[order]
    groups = (I % 40).astype(np.int64)
    groups[I % 11 == 0] = -1
    set_row_groups(s, I, groups)
    for flags in (1, 3):
        ref.check(s.neighbors_grouped(None, k, flags), ref.reference(oracle, R, I, groups, k, flags))
    sel = np.isin(np.arange(n), [i for i, r in enumerate(order) if r in set(where[2])])
    ref.check(s.neighbors_grouped([2], k, 3), ref.reference(oracle, R[sel], I[sel], groups[sel], k, 3))
    # hidden rows, a whole group among them
    part = np.ones(n, dtype=bool)
    part[groups == 5] = False
    part[[3, 4, 200]] = False
    assert (groups == 5).sum() >= 2
    s.hide_items(I[~part])
    for flags in (1, 2, 3):
        got = s.neighbors_grouped(None, k, flags)
        ref.check(got, ref.reference(oracle, R, I, groups, k, flags, part=part))
        assert not (got[3] == 5).any() and (got[4][~part] == 0).all()
    # a view against a fresh searcher of its rows; the view reads its parent's table at call time
    allowed = np.nonzero(rng.random(n) < 0.5)[0]
    v = s.view(I[allowed])
    fresh = build(ctx, R[allowed], I[allowed])  # (hidden rows keep their place in a view, too)
    fresh.hide_items(I[allowed][~part[allowed]])
    set_row_groups(fresh, I[allowed], groups[allowed])
    a, b = v.neighbors_grouped(None, k, 3), fresh.neighbors_grouped(None, k, 3)
    same(a, b)
    ref.check(a, ref.reference(oracle, R[allowed], I[allowed], groups[allowed], k, 3, part=part[allowed]))
    groups2 = (I % 9).astype(np.int64)
    set_row_groups(s, I, groups2)  # on the parent: the view's next call sees it
    ref.check(v.neighbors_grouped(None, k, 3), ref.reference(oracle, R[allowed], I[allowed], groups2[allowed], k, 3, part=part[allowed]))
    assert v.last_pair_group_stats()["grouped_rows"] == int(takes_part(R[allowed], part[allowed]).sum())
    v.close()
    fresh.close()
    # groups changed between two calls, rows removed
    ref.check(s.neighbors_grouped(None, k, 1), ref.reference(oracle, R, I, groups2, k, 1, part=part))
    s.unhide_items(I[~part])
    gone = [0, 33, n - 1]
    s.remove_items(I[gone])
    keep = np.setdiff1d(np.arange(n), gone)
    got = s.neighbors_grouped(None, k, 3)
    assert len(got[0]) == n - 3
    ref.check(got, ref.reference(oracle, R[keep], I[keep], groups2[keep], k, 3))
    s.close()


# ---- 9. match --------------------------------------------------------------------------------------------------------------------
SELECTIONS = {"disjoint": ([1], [2, 3]), "overlapping": ([1, 2], [2, 3]), "identical": ([2], [2]), "from before to": ([1], [3]), "from after to": ([3], [1])}


def test_match(ctx, oracle):
    rng = np.random.default_rng(9)
    n, k = 600, 6
    rows = rng.standard_normal((n, D)).astype(np.float32)
    src = np.repeat([1, 2, 3], [200, 250, 150])
    # ties across the sources, where the launch order of `match` is not the position order: one vector at five positions
    for p in (10, 210, 220, 460, 470):
        rows[p] = rows[10] * np.float32(2.0 ** (p % 3))
    rows[300] = 0.0
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    groups = (np.arange(n) % 50).astype(np.int64)  # every group has members in every source
    groups[::7] = -1
    groups[[10, 210, 220, 460]] = [1, 2, -1, 1]
    assert groups[470] not in (-1, 1, 2)
    s = build(ctx, rows, ids, sources=[(1, 0, 200), (2, 200, 450), (3, 450, 600)])
    set_row_groups(s, ids, groups)
    for case, (frm, to) in SELECTIONS.items():
        owner, partner = np.isin(src, frm), np.isin(src, to)
        for lo in (-1.0, 0.2):
            for flags in (1, 3):
                got = s.match_grouped(frm, to, k, lo, flags)
                want = ref.reference(oracle, rows, ids, groups, k, flags, owner, partner, lo)
                print(case, lo, flags)
                ref.check(got, want)
                st = s.last_match_stats()
                assert st["rows"] == int(owner.sum()) and st["partner_rows"] == int(partner.sum()) and st["listed"] == int(got[4].sum())
                if lo == 0.2:
                    assert got[4].min() < k
    # the tie, from behind the partners: owner 470 sees 10 (group 1), 210 (group 2), 220, 460 (group 1 again: collapsed under flags 3)
    got = s.match_grouped([3], [1, 2, 3], k, -1.0, 3)
    assert got[1][470 - 450, :3].tolist() == [ids[10], ids[210], ids[220]] and ids[460] not in got[1][470 - 450]
    got = s.match_grouped([3], [1, 2, 3], k, -1.0, 1)
    assert got[1][470 - 450, :4].tolist() == [ids[10], ids[210], ids[220], ids[460]]
    # an empty `to`
    e = s.match_grouped([1], [], k, -1.0, 3)
    assert len(e[0]) == 200 and (e[4] == 0).all() and (e[1] == -1).all() and (e[3] == -1).all()
    assert len(s.match_grouped([], [1], k, -1.0, 3)[0]) == 0
    s.close()


# ---- 10. today's workaround ----------------------------------------------------------------------------------------------------
def test_equals_the_host_filter(ctx):
    rng = np.random.default_rng(10)
    n, k = 3000, 10
    docs = rng.standard_normal((n // 8, D)).astype(np.float32)
    rows = np.ascontiguousarray((docs[np.arange(n) // 8] + 0.5 * rng.standard_normal((n, D))).astype(np.float32))
    ids = make_ids(rng, n)
    groups = (np.arange(n) // 8).astype(np.int64)
    assert np.bincount(groups).max() <= 8
    s = build(ctx, rows, ids)
    set_row_groups(s, ids, groups)
    wide = s.neighbors(None, k + 7)
    group_of_id = dict(zip(ids.tolist(), groups.tolist()))
    sib_in_top = 0
    f_ids = np.full((n, k), -1, dtype=np.int64)
    f_sc = np.full((n, k), np.nan, dtype=np.float32)
    for r in range(n):
        keep = [j for j in range(k + 7) if group_of_id[int(wide[1][r, j])] != groups[r]][:k]
        sib_in_top += (k + 7) - len([j for j in range(k + 7) if group_of_id[int(wide[1][r, j])] != groups[r]])
        f_ids[r], f_sc[r] = wide[1][r, keep], wide[2][r, keep]
    assert sib_in_top > 5 * n  # the siblings do fill the plain lists
    got = s.neighbors_grouped(None, k, SKIP)
    assert (got[4] == k).all()
    np.testing.assert_array_equal(got[1], f_ids)
    np.testing.assert_array_equal(bits(got[2]), bits(f_sc))
    np.testing.assert_array_equal(got[3], np.vectorize(group_of_id.get)(got[1]))
    assert s.last_pair_group_stats()["sibling_candidates"] >= sib_in_top
    s.close()


# ---- 11. duplicates ------------------------------------------------------------------------------------------------------------
def test_duplicates(ctx, oracle):
    rng = np.random.default_rng(11)
    n, thr = 2000, 0.9
    rows = rng.standard_normal((n, D)).astype(np.float32)
    groups = (np.arange(n) // 8).astype(np.int64)
    groups[::13] = -1
    planted = []
    for i, cos in enumerate((0.95, 0.9003, 0.8997, 0.85) * 6):
        a = 16 * i + 1
        sibling, foreign = a + 1, 1000 + 16 * i
        if groups[a] < 0 or groups[sibling] != groups[a]:
            continue
        rows[sibling] = neighbour(rng, rows[a], cos)
        rows[foreign] = neighbour(rng, rows[a], cos)
        planted.append((a, sibling, foreign, cos))
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    assert len(planted) >= 16
    want = ref.duplicates(oracle, rows, ids, groups, thr)
    plain = duplicates_ref.reference(oracle, rows, ids, thr)
    assert want[3] > 0 and len(want[0]) > 0 and len(want[0]) + want[3] == len(plain[0])
    above = sum(1 for *_x, cos in planted if cos > thr)
    assert want[3] >= above and len(want[0]) >= above  # sibling pairs and foreign pairs on both sides of the threshold
    s = build(ctx, rows, ids)
    set_row_groups(s, ids, groups)
    got = s.find_duplicates_grouped(None, thr)
    duplicates_ref.check(got[:4], want[:3])
    assert got[4] == want[3]
    p = s.find_duplicates(None, thr)
    assert got[3] + got[4] == p[3] == len(plain[0])
    st = s.last_pair_group_stats()
    assert st["flags"] == SKIP and st["sibling_candidates"] == got[4] and st["grouped_rows"] == int((groups >= 0).sum())
    few = s.find_duplicates_grouped(None, thr, max_pairs=3)
    duplicates_ref.check(few[:4], want[:3], 3)
    s.clear_groups()
    none = s.find_duplicates_grouped(None, thr)
    same(none[:3], p[:3])
    assert none[3] == p[3] and none[4] == 0
    s.close()


# ---- 12. stability -------------------------------------------------------------------------------------------------------------
def test_stability(ctx, oracle, golden_dir):
    rows, ids = golden(golden_dir, "scan_n1000_d384", "cosine")
    groups = (ids // 8).astype(np.int64)
    k = 10
    base = None
    for copy, kernel, tuning, cap in (("off", "auto", 0, None), ("int8", "auto", 32, 64), ("auto", "mfma", 0, 4096), ("auto", "wave", 32, None)):
        s = pa.Searcher(ctx, D, "cosine")
        s.set_screening_copy(copy)
        s.add_rows(1, rows[:500], ids[:500])
        s.add_rows(2, rows[500:], ids[500:])
        s.finalize()
        s.set_kernel(kernel)
        s.set_tuning(tuning)
        if cap:
            s.set_candidate_capacity(cap)
        before = (s.neighbors(None, k), s.match([1], [2], k, 0.0), s.reach_tree(None, 5))
        set_row_groups(s, ids, groups)
        runs = [(s.neighbors_grouped(None, k, 3), s.match_grouped([2], [1], k, -1.0, 3), s.find_duplicates_grouped(None, 0.3)) for _ in range(2)]
        for x, y in zip(runs[0], runs[1]):  # two runs give equal bits
            same([np.asarray(v) for v in x], [np.asarray(v) for v in y])
        if base is None:
            base = runs[0]
            ref.check(base[0], ref.reference(oracle, rows, ids, groups, k, 3))
        for x, y in zip(runs[0], base):  # ... and so does every search setting
            same([np.asarray(v) for v in x], [np.asarray(v) for v in y])
        after = (s.neighbors(None, k), s.match([1], [2], k, 0.0), s.reach_tree(None, 5))
        for x, y in zip(before, after):  # the plain calls are what they were
            same([np.asarray(v) for v in x], [np.asarray(v) for v in y])
        s.close()


def test_errors_on_the_device(ctx):
    s = build(ctx, np.ones((40, D), dtype=np.float32), np.arange(40, dtype=np.int64))
    with pytest.raises(ValueError):
        s.neighbors_grouped(None, 3, 4)
    with pytest.raises(ValueError):
        s.match_grouped(None, None, 65)
    s.add_rows(1, np.ones((1, D), dtype=np.float32), np.array([99], dtype=np.int64))  # pending rows: as the plain calls
    for call in (lambda: s.neighbors_grouped(None, 3), lambda: s.match_grouped(None, None, 3), lambda: s.find_duplicates_grouped(None, 0.9)):
        with pytest.raises(pa.PcvError) as e:
            call()
        assert e.value.status == 1
    s.close()


# ---- 13. the C++ mirror --------------------------------------------------------------------------------------------------------
def test_cpp_mirror_pair_groups_program():
    src = os.path.join(ROOT, "tests", "cpp", "pair_groups_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "pair_groups_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pair_groups_mirror_test: ok" in r.stdout
