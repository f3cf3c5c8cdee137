"""GPU: density clusters (pcv_searcher_density_clusters), through the Python mirror of the C ABI.  The reference of every check is
density_ref.py: the oracle's canonical cosine decides every pair at or near the threshold, and degrees, core rows, components,
their numbering and the border rule follow the definition in plain Python; ids, labels, kinds, degrees, the number of clusters and
the core / border / noise / cluster counters are compared for equality.  Each test first asserts on the CPU what makes its input
hostile: which pairs the bf16 screen decides alone, which fall into the band of its certified margin, which rows it is not
certified for."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from density_ref import BORDER, CORE, NOISE, NONE, canonical_norm2, check, cluster, margin, near_pairs, reference, takes_part
from duplicates_ref import bf16_rne, build, make_ids, neighbour, screen_score
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
F32_ACC = 1e-4  # more than the f32 accumulation and scaling error of the device's screening score, (Dp + 16) 2^-23 + 4 * 2^-24, at d <= 384


def f32_at_or_below(c):
    t = np.float32(c)
    return float(t) if float(t) <= c else float(np.nextafter(t, np.float32(-np.inf)))


def f32_above(c):
    t = np.float32(c)
    return float(t) if float(t) > c else float(np.nextafter(t, np.float32(np.inf)))


def screen_matrix(rows):
    """duplicates_ref.screen_score of every pair at once: the bf16-rounded rows' f64 Gram over the canonical norms"""
    b = bf16_rne(rows).astype(np.float64)
    nrm = np.sqrt(canonical_norm2(rows))
    return (b @ b.T) / np.outer(nrm, nrm)


def want_for(oracle, rows, ids, threshold, min_items, part=None):
    """reference(), keeping the near pairs so that several min_items share them"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    live = np.nonzero(takes_part(rows, part))[0]
    pairs = near_pairs(oracle, rows, threshold, live)

    def at(m):
        return (np.asarray(ids, dtype=np.int64).copy(),) + cluster(rows.shape[0], live, [(a, b) for a, b, _c in pairs], m)

    return at(min_items) if min_items is not None else at, pairs


# ---- a. a chain across tiles, segments and blocks ---------------------------------------------------------------------------------
CHAIN_SEED = {384: 7386, 64: 7064, 100: 7103}  # (corpora on which the CPU-side assertions below hold)


def chain_corpus(dim):
    """A random walk of 600 steps on the sphere, consecutive rows at cosine 0.95, norms scaled by U(0.5, 2), shuffled among 1 500
    Gaussian rows over three sources of 700, 777 and 623 rows.  -> rows, ids, sources, where[i]: the position of step i"""
    rng = np.random.default_rng(CHAIN_SEED[dim])
    steps, filler, c = 600, 1500, 0.95
    p = np.empty((steps, dim))
    p[0] = rng.standard_normal(dim)
    p[0] /= np.linalg.norm(p[0])
    for i in range(steps - 1):
        u = rng.standard_normal(dim)
        u -= (u @ p[i]) * p[i]
        u /= np.linalg.norm(u)
        p[i + 1] = c * p[i] + np.sqrt(1.0 - c * c) * u
        p[i + 1] /= np.linalg.norm(p[i + 1])
    n = steps + filler
    rows = rng.standard_normal((n, dim))
    where = np.sort(rng.permutation(n)[:steps])
    where = where[rng.permutation(steps)]  # the walk visits its positions in a random order
    rows[where] = p * rng.uniform(0.5, 2.0, size=(steps, 1))
    sources = [(1, 0, 700), (2, 700, 1477), (3, 1477, n)]
    return np.ascontiguousarray(rows.astype(np.float32)), make_ids(rng, n), sources, where


@pytest.mark.parametrize("dim", [384, 64, 100])
def test_chain_across_tiles_segments_and_blocks(ctx, oracle, dim):
    rows, ids, sources, where = chain_corpus(dim)
    n, thr, mg = rows.shape[0], 0.93, margin(dim)
    t = float(np.float32(thr))
    assert [hi - lo for _s, lo, hi in sources] == [700, 777, 623] and 777 % 32 and n == 2100
    # the links of the chain lie in many (tile, block) cells and cross the sources
    cells = {(min(a, b) // 128, max(a, b) // 32) for a, b in zip(where[:-1], where[1:])}
    src_of = np.searchsorted([700, 1477], where, side="right")
    assert len(cells) > 300 and (src_of[:-1] != src_of[1:]).sum() > 200
    S = screen_matrix(rows)
    R = rows.astype(np.float64)
    nrm = np.sqrt(canonical_norm2(rows))
    G = (R @ R.T) / np.outer(nrm, nrm)
    chain = np.zeros((n, n), dtype=bool)
    chain[where[:-1], where[1:]] = chain[where[1:], where[:-1]] = True
    np.fill_diagonal(G, -1.0)
    np.fill_diagonal(S, -1.0)
    # consecutive rows: 0.95000, and the screen sees them above t + margin whatever its rounding does
    assert np.abs(G[chain] - 0.95).max() < 1e-6 and S[chain].min() >= t + mg + F32_ACC
    want_at, pairs = want_for(oracle, rows, ids, thr, None)
    want = want_at(3)
    band = (S >= t - mg - F32_ACC) & (S < t + mg + F32_ACC) & np.triu(np.ones((n, n), dtype=bool), 1)
    in_band = {(int(a), int(b)) for a, b in zip(*np.nonzero(band))}
    confirmed = sum(1 for a, b, _c in pairs if (a, b) in in_band)
    print("%d-d: near pairs %d, in the band %d, of them near %d, largest other cosine %.4f" % (dim, len(pairs), len(in_band), confirmed, G[~chain].max()))
    if dim == 384:
        second = np.zeros((n, n), dtype=bool)
        second[where[:-2], where[2:]] = second[where[2:], where[:-2]] = True
        filler = np.ones(n, dtype=bool)
        filler[where] = False
        assert G[second].max() <= 0.9215 < t - mg and S[second].max() < t - mg - F32_ACC  # second neighbours: certainly below the band
        assert G[~chain & ~second].max() < 0.9 and G[filler].max() <= 0.24                 # everything else: far below
        assert len(pairs) == 599 and not in_band
        # one cluster: 598 core rows, the two ends (one partner each) border rows, the filler noise
        assert want[4] == 1 and (want[2] == CORE).sum() == 598 and (want[2] == BORDER).sum() == 2 and (want[2] == NOISE).sum() == 1500
        assert set(np.nonzero(want[2] == BORDER)[0].tolist()) == {int(where[0]), int(where[-1])}
    else:
        # some second neighbours fall into the band, and some of those are near: both paths feed one component
        strict = (S >= t - mg + F32_ACC) & (S < t + mg - F32_ACC) & np.triu(np.ones((n, n), dtype=bool), 1)
        surely_in_band = {(int(a), int(b)) for a, b in zip(*np.nonzero(strict))}
        surely_confirmed = sum(1 for a, b, _c in pairs if (a, b) in surely_in_band)
        assert len(surely_in_band) > 0 and 0 < surely_confirmed and confirmed < len(surely_in_band)
        assert want[4] == 1
    s = build(ctx, rows, ids, sources=sources)
    assert s.num_segments == 3
    got = s.density_clusters(None, thr, 3)
    st = s.last_density_stats()
    print(st)
    check(got, want, st)
    if dim == 384:
        assert st["sure_pairs"] == 599 and st["candidates"] == 0 and st["confirmed"] == 0
    else:
        assert st["candidates"] > 0 and 0 < st["confirmed"] < st["candidates"]
    assert st["tile_rows"] == 128 and st["reruns"] == 0
    # another min_items on the same pairs, and the sources in another order and one at a time
    check(s.density_clusters(None, thr, 2), want_at(2), s.last_density_stats())
    check(s.density_clusters([3, 1, 2], thr, 3), want, s.last_density_stats())
    lo, hi = sources[1][1], sources[1][2]
    check(s.density_clusters([2], thr, 3), reference(oracle, rows[lo:hi], ids[lo:hi], thr, 3), s.last_density_stats())
    s.close()


# ---- b. the edge of the margin, both sides ----------------------------------------------------------------------------------------
DOWN = 1.0 + 2.0 ** -8 - 2.0 ** -18  # exact in f32; halfway between two bf16 values less 2^-18: rounds down to 1
UP = 1.0 + 2.0 ** -8 + 2.0 ** -18    # rounds up to 1 + 2^-7
N_BIASED = 12                        # pairs of each kind


def biased_pair(rng, dim, mant, share):
    """a: features +-2^e * mant, e in -2..1; b: the same signs and mantissa with the exponents of `share` of the features redrawn
    (test_duplicates_paths_gpu.py): every feature of both rows rounds to bf16 in the same direction"""
    e = rng.integers(-2, 2, size=dim)
    sign = rng.choice([-1.0, 1.0], size=dim)
    m = min(dim, max(1, int(round(dim * share))))
    e2 = e.copy()
    where = rng.permutation(dim)[:m]
    e2[where] = (e[where] + 2 + rng.integers(1, 4, size=m)) % 4 - 2  # another exponent of the four
    a = (sign * np.ldexp(mant, e)).astype(np.float32)
    b = (sign * np.ldexp(mant, e2)).astype(np.float32)
    assert (a.astype(np.float64) == sign * np.ldexp(mant, e)).all() and (b.astype(np.float64) == sign * np.ldexp(mant, e2)).all()
    return a, b


@pytest.mark.parametrize("dim", [64, 384])
def test_edge_of_the_margin_both_sides(ctx, oracle, dim):
    rng = np.random.default_rng(100 + dim)
    n = 400
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    shares = np.linspace(1.0 / 64, 1.0 / 6, N_BIASED)  # cosines from about 0.9 to 1
    made = [("down", DOWN, sh) for sh in shares] + [("up", UP, sh) for sh in shares]
    places = rng.permutation(n)[: 2 * len(made)]
    pairs = {"down": [], "up": []}
    for i, (kind, mant, sh) in enumerate(made):
        a, b = sorted((int(places[2 * i]), int(places[2 * i + 1])))
        rows[a], rows[b] = biased_pair(rng, dim, mant, sh)
        pairs[kind].append((a, b))
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    pairs = {k: sorted(((a, b, oracle.canonical_score(rows[a], rows[b], 0)) for a, b in v), key=lambda x: x[2]) for k, v in pairs.items()}
    s = build(ctx, rows, ids)

    def three(kind):
        v = pairs[kind]
        return [v[0], v[len(v) // 2], v[-1]]

    # a down pair AT the threshold: the screen sees it nearly 0.00776 c below, inside the band, and the pair must not be lost
    for a, b, c in three("down"):
        thr = f32_at_or_below(c)
        sc = screen_score(rows[a], rows[b])
        print("down: c %.6f threshold %.6f screen %.6f" % (c, thr, sc))
        assert c >= thr and sc < thr - 0.0076 * c
        got = s.density_clusters(None, thr, 2)
        st = s.last_density_stats()
        check(got, reference(oracle, rows, ids, thr, 2), st)
        assert got[2][a] == CORE and got[2][b] == CORE and got[1][a] == got[1][b] >= 0 and got[3][a] >= 1
        assert st["confirmed"] >= 1
    # an up pair just BELOW the threshold: the screen sees it nearly 0.00779 c above — at or above the threshold, but short of
    # threshold + margin — so it must not be counted as sure
    for a, b, c in three("up"):
        thr = f32_above(c)
        sc = screen_score(rows[a], rows[b])
        print("up: c %.6f threshold %.6f screen %.6f" % (c, thr, sc))
        assert c < thr <= 1.0 and sc >= thr and sc > c + 0.0077 * c
        got = s.density_clusters(None, thr, 2)
        st = s.last_density_stats()
        want = reference(oracle, rows, ids, thr, 2)
        check(got, want, st)
        assert (a, b) not in {(x, y) for x, y, _c in reference.pairs}
        assert got[1][a] != got[1][b] or got[1][a] == -1
        assert st["candidates"] > st["confirmed"]
    s.close()


# ---- c. more than one span --------------------------------------------------------------------------------------------------------
def span_corpus():
    """12 320 x 64: 385 blocks (test_duplicates_paths_gpu.py).  A work item streams 256 blocks from its tile's first block, so the
    tiles that start before block 129 have a second span.  Groups of (block, row of the block): the first is the base, the others
    copies ('c') or neighbours at 0.999 ('n') of it, on both sides of the span cut of the base's tile."""
    rng = np.random.default_rng(21)
    n, dim = 12320, 64
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    plan = [
        ((0, 5), [(255, 31, "c"), (256, 0, "n"), (384, 17, "n")]),    # tile of block 0: cut between blocks 255 and 256
        ((4, 7), [(259, 31, "n"), (260, 0, "c")]),                    # tile of block 4: cut between 259 and 260
        ((128, 0), [(383, 12, "c"), (384, 3, "n")]),                  # tile of block 128: its second span is the last block alone
        ((200, 20), [(300, 11, "n")]),                                # a tile with one span
        ((384, 25), [(384, 26, "c")]),                                # inside the last block
    ]
    groups = []
    for (bb, br), partners in plan:
        base = bb * 32 + br
        g = [base]
        for pb, pr, kind in partners:
            at = pb * 32 + pr
            rows[at] = rows[base] if kind == "c" else neighbour(rng, rows[base], 0.999)
            g.append(at)
        groups.append(sorted(g))
    return np.ascontiguousarray(rows), make_ids(rng, n), groups


def test_more_than_one_span(ctx, oracle):
    rows, ids, groups = span_corpus()
    n = rows.shape[0]
    assert n == 385 * 32 and [len(g) for g in groups] == [4, 3, 3, 2, 2]
    for g in groups:  # (two neighbours of one row are at 0.998 of each other)
        for a, b in itertools.combinations(g, 2):
            assert oracle.canonical_score(rows[a], rows[b], 0) >= 0.995
        assert g[0] // 32 + 256 <= g[-1] // 32 or g[0] // 32 >= 200  # the group straddles the cut of its base's tile, or has one span
    want_at, pairs = want_for(oracle, rows, ids, 0.99, None)
    assert sorted((a, b) for a, b, _c in pairs) == sorted(p for g in groups for p in itertools.combinations(g, 2))
    s = build(ctx, rows, ids)
    for m in (4, 3, 2):  # min_items = the group size: the groups of that size and above are clusters of core rows, the smaller noise
        want = want_at(m)
        big = sorted((g for g in groups if len(g) >= m), key=lambda g: g[0])
        assert want[4] == len(big)
        for j, g in enumerate(big):
            assert (want[1][g] == j).all() and (want[2][g] == CORE).all()
        got = s.density_clusters(None, 0.99, m)
        st = s.last_density_stats()
        check(got, want, st)
        assert st["reruns"] == 0 and st["rows"] == n and st["tile_rows"] == 128
    s.close()


# ---- d. cross-check against the duplicate pairs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_agrees_with_find_duplicates(ctx, oracle, golden_dir, metric):
    g = np.load(os.path.join(golden_dir, "scan_n1000_d384.npz"))
    rows = np.array(g["corpus"], dtype=np.float32)
    rng = np.random.default_rng(31)
    n = rows.shape[0]
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(n, 1))).astype(np.float32)
    spots = rng.permutation(n)[:90]
    for j in range(30):  # copies, scaled copies and close neighbours, some of them chained into groups of three
        a, b, c = (int(x) for x in spots[3 * j : 3 * j + 3])
        rows[b] = rows[a] if j % 3 == 0 else rows[a] * np.float32(0.5) if j % 3 == 1 else neighbour(rng, rows[a], 0.97)
        if j % 2:
            rows[c] = neighbour(rng, rows[b], 0.96)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    thr = 0.9
    s = build(ctx, rows, ids, metric)
    id_a, id_b, _scores, total = s.find_duplicates(None, thr)
    assert total == len(id_a) >= 45
    dup_ids, dup_group = pa.duplicate_groups(id_a, id_b)
    groups = {}
    for i, gid in zip(dup_ids.tolist(), dup_group.tolist()):
        groups.setdefault(gid, set()).add(i)
    assert any(len(v) >= 3 for v in groups.values())
    # min_items 1: every participating row is core, and the clusters of more than one row are the groups of duplicates
    got = s.density_clusters(None, thr, 1)
    st = s.last_density_stats()
    check(got, reference(oracle, rows, ids, thr, 1), st)
    assert st["border"] == 0 and st["noise"] == 0
    members = {}
    for i, lab in zip(got[0].tolist(), got[1].tolist()):
        if lab >= 0:
            members.setdefault(lab, set()).add(i)
    assert sorted(sorted(v) for v in members.values() if len(v) > 1) == sorted(sorted(v) for v in groups.values())
    assert st["sure_pairs"] + st["confirmed"] == total
    # min_items 2: a row is core iff it is in a pair
    got = s.density_clusters(None, thr, 2)
    check(got, reference(oracle, rows, ids, thr, 2), s.last_density_stats())
    np.testing.assert_array_equal(got[2] == CORE, np.isin(got[0], dup_ids))
    s.close()


# ---- e. rows that take no part ----------------------------------------------------------------------------------------------------
def test_rows_that_take_no_part(ctx, oracle):
    rng = np.random.default_rng(41)
    n, dim, thr = 500, 384, 0.95
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    ids = make_ids(rng, n)
    # groups of four: a base, a copy, a copy of norm about 2^30 and one of about 2^-30 (both outside the certified f32 screen)
    spots = rng.permutation(np.arange(10, n))[:40].reshape(10, 4)
    for base, cp, big, small in spots:
        rows[cp] = rows[base]
        rows[big] = np.ldexp(rows[base], 26)    # |x| about 2^4.3 * 2^26
        rows[small] = np.ldexp(rows[base], -35)
    rows[3] = 0.0            # no cosine
    rows[5, 17] = np.nan     # unsearchable
    rows = np.ascontiguousarray(rows)
    n2 = canonical_norm2(rows)
    wild = np.concatenate([spots[:, 2], spots[:, 3]])
    assert (n2[spots[:, 2]] > 2.0 ** 40).all() and (n2[spots[:, 3]] < 2.0 ** -40).all() and (n2[spots[:, 3]] > 2.0 ** -126).all()
    live = takes_part(rows)
    assert not live[3] and not live[5] and live.sum() == n - 2
    s = build(ctx, rows, ids)
    for m in (1, 4, 5):
        got = s.density_clusters(None, thr, m)
        st = s.last_density_stats()
        check(got, reference(oracle, rows, ids, thr, m), st)
        assert got[2][3] == NONE and got[2][5] == NONE and got[1][3] == -1 and got[3][5] == 0
        # every pair with a wild row goes through the f64 step
        assert st["candidates"] >= len(wild) * (n - 2 - len(wild)) and st["confirmed"] >= 5 * 10
        if m == 4:  # the wild rows are clustered with their copies
            for grp in spots:
                assert (got[2][grp] == CORE).all() and len(set(got[1][grp].tolist())) == 1 and (got[3][grp] == 3).all()
            assert got[4] == 10 and st["noise"] == n - 2 - 40
    # hidden ids: two whole groups, one member of a third, and a filler row
    hidden = np.concatenate([spots[0], spots[1], spots[2][:1], [0]])
    s.hide_items(ids[hidden])
    part = np.ones(n, dtype=bool)
    part[hidden] = False
    got = s.density_clusters(None, thr, 4)
    check(got, reference(oracle, rows, ids, thr, 4, part), s.last_density_stats())
    assert (got[2][hidden] == NONE).all() and got[4] == 7 and (got[2][spots[2][1:]] == NOISE).all()
    check(s.density_clusters(None, thr, 3), reference(oracle, rows, ids, thr, 3, part), s.last_density_stats())
    s.unhide_items(ids[hidden])
    # removed ids: the rows behind them move up
    gone = np.concatenate([spots[3][:2], [1, 2, n - 1]])
    assert s.remove_items(ids[gone]) == len(gone)
    keep = np.setdiff1d(np.arange(n), gone)
    got = s.density_clusters(None, thr, 2)
    check(got, reference(oracle, rows[keep], ids[keep], thr, 2), s.last_density_stats())
    assert len(got[0]) == n - len(gone) and got[4] == 10
    s.close()


# ---- f. a view --------------------------------------------------------------------------------------------------------------------
def test_view_clusters_its_own_rows(ctx, oracle):
    rng = np.random.default_rng(51)
    n, dim, thr = 600, 100, 0.9
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    centres = rng.permutation(n)[:6]
    for cidx in centres:  # topics of 30 rows at 0.96 of a centre: about 0.92 of each other
        members = rng.permutation(n)[:30]
        for r in members:
            if r not in centres:
                rows[r] = neighbour(rng, rows[cidx], 0.96)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids, sources=[(1, 0, 250), (2, 250, n)])
    whole = s.density_clusters(None, thr, 5)
    check(whole, reference(oracle, rows, ids, thr, 5), s.last_density_stats())
    assert whole[4] >= 3 and (whole[2] == BORDER).sum() + (whole[2] == NOISE).sum() > 300
    allowed = np.nonzero(rng.random(n) < 0.5)[0]
    v = s.view(ids[allowed])
    got = v.density_clusters(None, thr, 5)
    check(got, reference(oracle, rows[allowed], ids[allowed], thr, 5), v.last_density_stats())
    assert (got[3] <= whole[3][allowed]).all() and (got[3] < whole[3][allowed]).sum() > 20  # fewer partners: the degrees drop
    in2 = allowed[allowed >= 250]
    check(v.density_clusters([2], thr, 5), reference(oracle, rows[in2], ids[in2], thr, 5), v.last_density_stats())
    v.close()
    s.close()


# ---- g. degenerate sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 33, 129])
def test_degenerate_sizes(ctx, oracle, n):
    rng = np.random.default_rng(600 + n)
    dim = 64
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    if n > 1:
        rows[n - 1] = rows[0]                            # the last row (alone in its block or tile) is a copy of the first
        rows[n // 2] = rows[0] * np.float32(3.0)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids)
    for thr in (1.0, BELOW_ONE, 0.3, -0.999):
        for m in (1, 2, 3, n + 1):
            got = s.density_clusters(None, thr, m)
            check(got, reference(oracle, rows, ids, thr, m), s.last_density_stats())
    got = s.density_clusters(None, BELOW_ONE, 3)
    if n > 2:  # the three copies: one cluster at the f32 just below 1
        assert got[4] == 1 and sorted(np.nonzero(got[2] == CORE)[0].tolist()) == sorted({0, n // 2, n - 1})
    else:
        assert got[4] == 0 and got[2].tolist() == [NOISE]
    # an empty source list: n = 0 and nothing is launched
    empty = s.density_clusters([], 0.5, 2)
    assert all(len(x) == 0 for x in empty[:4]) and empty[4] == 0
    st = s.last_density_stats()
    assert st["rows"] == 0 and st["prep_ms"] == 0 and st["degree_ms"] == 0 and st["tile_rows"] == 0
    assert all(len(x) == 0 for x in s.density_clusters([99], 0.5, 2)[:4])
    s.close()


# ---- h. independence and repeatability --------------------------------------------------------------------------------------------
def test_independent_of_settings_and_repeatable(ctx, oracle):
    rows, ids, sources, _where = chain_corpus(100)
    want = reference(oracle, rows, ids, 0.93, 3)
    first = None
    for copy, kernel, flags, cap in (("off", "auto", 0, None), ("int8", "mfma", 32, 64), ("auto", "auto", 0, 4096)):
        s = pa.Searcher(ctx, rows.shape[1], "cosine")
        s.set_screening_copy(copy)
        for sid, lo, hi in sources:
            s.add_rows(sid, rows[lo:hi], ids[lo:hi])
        s.finalize()
        s.set_kernel(kernel)
        s.set_tuning(flags)
        if cap:
            s.set_candidate_capacity(cap)
        a = s.density_clusters(None, 0.93, 3)
        s.search_vectors(None, 5, rows[:3])  # a search in between leaves its pass state behind; the next call does not see it
        b = s.density_clusters(None, 0.93, 3)
        check(a, want, s.last_density_stats())
        first = first or a
        for x, y, z in zip(a[:4], b[:4], first[:4]):
            assert x.tobytes() == y.tobytes() == z.tobytes()
        assert a[4] == b[4] == first[4]
        s.close()


def test_band_list_rerun(ctx, oracle):
    """700 rows at 0.9747 of one centre: about 0.95 of each other, within a few thousandths — nearly every pair lies in the band
    of the screen's margin around 0.95, four times the list's first room of max(65536, 2 rows)."""
    rng = np.random.default_rng(71)
    n, dim, thr = 800, 384, 0.95
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    centre = rng.standard_normal(dim).astype(np.float32)
    for r in range(700):
        rows[r] = neighbour(rng, centre, np.sqrt(0.95))
    order = rng.permutation(n)
    rows = np.ascontiguousarray(rows[order])
    ids = make_ids(rng, n)
    t, mg = float(np.float32(thr)), margin(dim)
    S = screen_matrix(rows)
    surely_band = ((S >= t - mg + F32_ACC) & (S < t + mg - F32_ACC) & np.triu(np.ones((n, n), dtype=bool), 1)).sum()
    print("pairs surely in the band: %d" % surely_band)
    assert surely_band > 3 * max(65536, 2 * n)
    want_at, pairs = want_for(oracle, rows, ids, thr, None)
    assert 50000 < len(pairs) < 200000
    s = build(ctx, rows, ids)
    for m in (300, 2):
        got = s.density_clusters(None, thr, m)
        st = s.last_density_stats()
        print(st)
        check(got, want_at(m), st)
        assert st["reruns"] == 1 and st["candidates"] >= surely_band and 0 < st["confirmed"] < st["candidates"]
    s.close()


# ---- i. argument errors that need the searcher ------------------------------------------------------------------------------------
def test_argument_errors_on_the_device(ctx):
    rng = np.random.default_rng(81)
    n = 40
    s = build(ctx, rng.standard_normal((n, 64)).astype(np.float32), np.arange(n, dtype=np.int64))
    ids = np.full(n, -77, dtype=np.int64)
    label = np.full(n, -77, dtype=np.int32)
    kind = np.full(n, -77, dtype=np.int8)
    degree = np.full(n, -77, dtype=np.int32)
    rows, clusters = C.c_int64(-5), C.c_int32(-5)

    def raw(capacity, arrays=True):
        p = (_ffi.i64p(ids), _ffi.i32p(label), _ffi.i8p(kind), _ffi.i32p(degree)) if arrays else (None, None, None, None)
        return _ffi.lib().pcv_searcher_density_clusters(s._handle, None, 0, 0.5, 2, capacity, p[0], p[1], p[2], p[3], C.byref(rows),
                                                        C.byref(clusters) if arrays else None)

    assert raw(n) == 0 and rows.value == n and (kind == NOISE).all() and clusters.value == 0
    assert s.last_density_stats()["rows"] == n and s.last_density_stats()["prep_ms"] > 0
    # the count alone: no device work, the stats are zero
    rows.value = -5
    assert raw(0, arrays=False) == 0 and rows.value == n
    st = s.last_density_stats()
    assert all(v == 0 for v in st.values()), st
    # capacity < n: PCV_ERR_INVALID with out_rows set and nothing else written
    label[:] = -77
    rows.value = -5
    for cap in (n - 1, 1):
        assert raw(cap) == 1 and rows.value == n and "room for %d rows" % cap in _ffi.lib().pcv_last_error().decode()
        assert (label == -77).all()
    # out_ids and out_degree may be NULL
    assert _ffi.lib().pcv_searcher_density_clusters(s._handle, None, 0, 0.5, 1, n, None, _ffi.i32p(label), _ffi.i8p(kind), None, C.byref(rows),
                                                    C.byref(clusters)) == 0
    assert clusters.value == n and (kind == CORE).all() and sorted(label.tolist()) == list(range(n))
    with pytest.raises(ValueError):
        s.density_clusters(None, 1.5, 2)
    with pytest.raises(ValueError):
        s.density_clusters(None, 0.5, 0)
    s.set_shard_offset(5)  # a sharded searcher
    with pytest.raises(pa.PcvError) as e:
        s.density_clusters(None, 0.5, 2)
    assert e.value.status == 1 and "sharded" in str(e.value)
    s.set_shard_offset(0)
    assert s.density_clusters(None, 0.5, 2)[4] == 0
    s.add_rows(1, np.ones((1, 64), dtype=np.float32), np.array([99], dtype=np.int64))  # pending rows: as a search
    with pytest.raises(pa.PcvError) as e:
        s.density_clusters(None, 0.5, 2)
    assert e.value.status == 1
    s.close()


# ---- j. the C++ mirror ------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_density_program(oracle, golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "scan_n77_d100.npz"))
    rows = np.array(g["corpus"], dtype=np.float32)
    rng = np.random.default_rng(91)
    for base, others in ((4, (20, 33, 64)), (10, (11, 76)), (50, (51,))):
        for r in others:
            rows[r] = neighbour(rng, rows[base], 0.97)
    rows[40] = 0.0
    rows = np.ascontiguousarray(rows)
    n, dim = rows.shape
    ids = 5000 + 3 * np.arange(n, dtype=np.int64)
    thr, m = np.float32(0.9), 3
    want = reference(oracle, rows, ids, float(thr), m)
    assert want[4] == 2 and (want[2] == CORE).sum() == 7 and (want[2] == NONE).sum() == 1
    raw = tmp_path / "rows.f32"
    rows.astype("<f4").tofile(str(raw))
    args = [str(raw), str(n), str(dim), "%08x" % int(np.array([thr]).view(np.uint32)[0]), str(m), str(want[4])]
    for i in range(n):
        args += [str(int(want[1][i])), str(int(want[2][i])), str(int(want[3][i]))]
    src = os.path.join(ROOT, "tests", "cpp", "density_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "density_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "density_mirror_test: ok" in r.stdout
