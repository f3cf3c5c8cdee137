"""GPU: the linkage tree (pcv_searcher_linkage_tree), through the Python mirror of the C ABI.  The reference of every check is
linkage_ref.py: Kruskal over every participating pair scored by the oracle's canonical cosine for corpora of up to 700 rows, and for
larger ones the verifier that replays the returned edges; positions, ids, the f64 bits of c, out_part, the edge count and the stats
counters are compared for equality.  Each test first asserts on the CPU what makes its input hostile: ties the edge order must
break, screening scores that sit between one and two margins below a component's bound, best partners in blocks the bound pass
does not sample, rows the screen is not certified for, more candidates than the list's first room."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from density_ref import canonical_norm2, margin, takes_part
from duplicates_ref import bf16_rne, build, make_ids, neighbour, screen_score
from linkage_ref import check, check_verified, cut, reference
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
F32_ACC = 1e-4  # more than the f32 accumulation and scaling error of the device's screening score, (Dp + 16) 2^-23 + 4 * 2^-24, at d <= 384


def screen_matrix(rows):
    """duplicates_ref.screen_score of every pair at once: the bf16-rounded rows' f64 Gram over the canonical norms"""
    b = bf16_rne(rows).astype(np.float64)
    nrm = np.sqrt(canonical_norm2(rows))
    return (b @ b.T) / np.outer(nrm, nrm)


def cosine_matrix(rows):
    r = rows.astype(np.float64)
    nrm = np.sqrt(canonical_norm2(rows))
    return (r @ r.T) / np.outer(nrm, nrm)


def same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def log2_ceil(p):
    return int(np.ceil(np.log2(max(p, 1))))


# ---- a. golden corpora ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("name,first", [("scan_n77_d100", 77), ("scan_n1000_d384", 600)])
def test_golden(ctx, oracle, golden_dir, name, first, metric):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    rows = np.array(g["corpus"], dtype=np.float32)[:first]
    rng = np.random.default_rng(21)
    if metric == "dot":  # rows of several lengths: the tree is by cosine all the same
        rows = (rows * rng.uniform(0.5, 1.5, size=(rows.shape[0], 1))).astype(np.float32)
    rows = np.ascontiguousarray(rows)
    n = rows.shape[0]
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids, metric)
    got = s.linkage_tree(None)
    st = s.last_linkage_stats()
    print(st)
    check(got, reference(oracle, rows, ids), st)
    assert st["tile_rows"] == 128 and st["reruns"] == 0
    s.close()


# ---- b. ties ----------------------------------------------------------------------------------------------------------------------
def test_ties_the_star(ctx, oracle):
    """64 orthonormal directions at 64-d: every c is exactly 0 (and every screening score), so the positions alone order the edges.
    Every row but the first chooses (0, r), row 0 chooses (0, 1): one round, and every foreign pair was a candidate of it."""
    rows = np.ascontiguousarray(np.eye(64, dtype=np.float32)[:, ::-1] * np.float32(3.0))
    ids = np.arange(64, dtype=np.int64) * 5 + 2
    G = cosine_matrix(rows)
    assert (G[~np.eye(64, dtype=bool)] == 0.0).all() and (screen_matrix(rows)[~np.eye(64, dtype=bool)] == 0.0).all()
    want = reference(oracle, rows, ids)
    assert want[2].tolist() == [0] * 63 and want[3].tolist() == list(range(1, 64)) and (want[6] == 0.0).all()
    s = build(ctx, rows, ids)
    got = s.linkage_tree(None)
    st = s.last_linkage_stats()
    check(got, want, st)
    assert st["rounds"] == 1 and st["candidates"] == 64 * 63
    s.close()


def test_ties_identical_rows_and_cosines_1e_10_apart(ctx, oracle):
    rng = np.random.default_rng(32)
    dim = 100
    # four groups of 16 identical rows, shuffled over two segments: every c inside a group has the same bits, and so has every c
    # between two groups
    base = rng.standard_normal((4, dim)).astype(np.float32)
    group = rng.permutation(np.repeat(np.arange(4), 16))
    rows = np.ascontiguousarray(base[group])
    ids = make_ids(rng, 64)
    want = reference(oracle, rows, ids)
    inside = group[want[2]] == group[want[3]]
    assert inside[:60].all() and not inside[60:].any() and (want[6][:60] > 0.999999).all()  # 15 edges inside each group, then three
    for g in range(4):  # ... of one value each: the positions alone order them
        assert len(set(want[6][inside & (group[want[2]] == g)].tolist())) == 1
    s = build(ctx, rows, ids, sources=[(1, 0, 29), (2, 29, 64)])
    assert s.num_segments == 2
    got = s.linkage_tree(None)
    check(got, want, s.last_linkage_stats())
    s.close()
    # families (b, p, p'): p at 0.9 of b, p' = p with one feature moved by an ulp.  p and p' join first; then the family's edge to
    # b is (b, p) or (b, p'), and the two cosines differ by about 1e-10
    n, fam = 600, 100
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    spots = rng.permutation(n)[: 3 * fam].reshape(fam, 3)
    gaps = []
    for b, p, q in spots:
        rows[p] = neighbour(rng, rows[b], 0.9)
        rows[q] = rows[p]
        # (an ulp of feature j moves the cosine by about |b_j - 0.9 p_j| ulp(p_j) / |b|^2, |p| = |b|: the feature that brings it nearest 1e-10)
        effect = np.abs(rows[b].astype(np.float64) - 0.9 * rows[p].astype(np.float64)) * np.spacing(np.abs(rows[p])).astype(np.float64) / float(canonical_norm2(rows[b : b + 1])[0])
        j = int(np.argmin(np.abs(effect - 1e-10)))
        rows[q, j] = np.nextafter(rows[q, j], np.float32(np.inf))
        gaps.append(abs(oracle.canonical_score(rows[b], rows[p], 0) - oracle.canonical_score(rows[b], rows[q], 0)))
    rows = np.ascontiguousarray(rows)
    gaps = np.array(gaps)
    print("gaps %.3g .. %.3g" % (gaps.min(), gaps.max()))
    assert (gaps > 5e-11).all() and (gaps < 2e-10).all()
    ids = make_ids(rng, n)
    want = reference(oracle, rows, ids)
    s = build(ctx, rows, ids)
    got = s.linkage_tree(None)
    check(got, want, s.last_linkage_stats())
    s.close()


# ---- c. many rounds: a chain across tiles, segments and blocks --------------------------------------------------------------------
CHAIN_SEED = {384: 7386, 64: 7064, 100: 7103}


def chain_corpus(dim):
    """The chain corpus of test_density_gpu.py: a random walk of 600 steps on the sphere, consecutive rows at cosine 0.95, norms
    scaled by U(0.5, 2), shuffled among 1 500 Gaussian rows over three sources of 700, 777 and 623 rows."""
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
def test_chain_many_rounds(ctx, oracle, dim):
    rows, ids, sources, where = chain_corpus(dim)
    n = rows.shape[0]
    G = cosine_matrix(rows)
    np.fill_diagonal(G, -1.0)
    # what is hostile: the 599 links (0.95) are tree edges whose ends lie in many (tile, block) cells and in different sources, and
    # a row of the walk has two of them: components grow along the chain, not by pairs of rows alone
    links = G[where[:-1], where[1:]]
    assert np.abs(links - 0.95).max() < 1e-6
    cells = {(min(a, b) // 128, max(a, b) // 32) for a, b in zip(where[:-1], where[1:])}
    assert len(cells) > 300
    s = build(ctx, rows, ids, sources=sources)
    assert s.num_segments == 3
    got = s.linkage_tree(None)
    st = s.last_linkage_stats()
    print(st)
    check_verified(oracle, rows, ids, got, None, st)
    assert 3 <= st["rounds"] <= log2_ceil(n) and st["participating"] == n
    in_tree = set(zip(got[2].tolist(), got[3].tolist()))
    chain_links = {(int(min(a, b)), int(max(a, b))) for a, b in zip(where[:-1], where[1:])}
    if dim == 384:  # every other cosine of a walk row is far below 0.95: all the links are in the tree
        assert chain_links <= in_tree
    # the sources in another order and one at a time
    same_bits(s.linkage_tree([3, 1, 2]), got)
    lo, hi = sources[1][1], sources[1][2]
    check_verified(oracle, rows[lo:hi], ids[lo:hi], s.linkage_tree([2]), None, s.last_linkage_stats())
    s.close()


# ---- d. the 2 m slack -------------------------------------------------------------------------------------------------------------
DOWN = 1.0 + 2.0 ** -8 - 2.0 ** -18  # exact in f32; halfway between two bf16 values less 2^-18: rounds down to 1
UP = 1.0 + 2.0 ** -8 + 2.0 ** -18    # rounds up to 1 + 2^-7


def kruskal(G):
    """the tree of a dense symmetric weight matrix under the edge order, by positions"""
    n = G.shape[0]
    a, b = np.triu_indices(n, 1)
    order = np.lexsort((b, a, -G[a, b]))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    tree = set()
    for i in order:
        x, y = find(int(a[i])), find(int(b[i]))
        if x != y:
            parent[max(x, y)] = min(x, y)
            tree.add((int(a[i]), int(b[i])))
    return tree


def boruvka(G, S, slack):
    """Borůvka rounds on the CPU as the device runs them, in exact arithmetic: a component's bound is its largest screening score
    S with a foreign row, its candidates are the foreign pairs with S >= bound - slack, and the true weights G choose among them.
    -> the edges chosen.  It shows what a smaller slack would do to an input; it is never an expected result."""
    n = G.shape[0]
    comp = np.arange(n)
    edges = set()
    while len(set(comp.tolist())) > 1:
        foreign = comp[:, None] != comp[None, :]
        choice = {}
        for root in sorted(set(comp.tolist())):
            mine = comp == root
            Sm = np.where(foreign[mine], S[mine], -np.inf)
            listed = Sm >= Sm.max() - slack
            Gm = np.where(listed, G[mine], -np.inf)
            best = Gm.max()
            rows_m = np.nonzero(mine)[0]
            pairs = sorted((min(int(rows_m[i]), int(j)), max(int(rows_m[i]), int(j))) for i, j in zip(*np.nonzero(Gm == best)))
            choice[root] = pairs[0]
        before = len(set(comp.tolist()))
        for a, b in choice.values():
            edges.add((a, b))
            ca, cb = comp[a], comp[b]
            if ca != cb:
                comp[comp == max(ca, cb)] = min(ca, cb)
        assert len(set(comp.tolist())) < before
    return edges


def away_from(rng, a, cos, avoid):
    """a row at cosine `cos` of a whose other part is orthogonal to a and to every row of `avoid`: its cosine with each of those is
    cos times a's"""
    basis = []
    for v in [a] + list(avoid):
        v = v.astype(np.float64).copy()
        for w in basis:
            v -= (v @ w) * w
        if np.linalg.norm(v) > 1e-9:
            basis.append(v / np.linalg.norm(v))
    u = rng.standard_normal(a.shape[0])
    for w in basis:
        u -= (u @ w) * w
    u /= np.linalg.norm(u)
    a64 = a.astype(np.float64)
    return ((cos * a64 / np.linalg.norm(a64) + np.sqrt(1.0 - cos * cos) * u) * np.linalg.norm(a64)).astype(np.float32)


def slack_case(oracle, dim, several):
    """The owner O has half its features at UP and half at DOWN (the biased rows of test_neighbors_gpu.py).  U lives on the first
    half with the value UP: the screen sees c(O, U) 0.0055 too high.  Dn lives on the second half with the value DOWN, and one small
    feature of the first half lifts c(O, Dn) just above c(O, U), both about 0.71: Dn is O's best partner, and the screen sees it
    0.0055 too low.  The gap of the two screening scores lies between m and 2 m: U sets the bound of O's component, and a slack of
    m, or a conversion rounded the wrong way, loses the edge (O, Dn).
    Losing it must show in the tree, so (O, U) must not be a tree edge: Dn and U are joined by a chain of six rows in steps of 30
    degrees (0.866) through a direction orthogonal to both halves, every row of it below 0.62 of O.  The tree holds the chain and
    (O, Dn); a round that lists (O, U) and not (O, Dn) — from O's side, or from the chain's once it holds U and Dn — emits (O, U).
    several: O is not alone when it chooses.  T at 0.97 of O joins it in round 0; P at 0.93 of O and Q at 0.97 of P join each
    other in round 0 and {O, T} in round 1: from round 2 on the component {O, T, P, Q} looks for its best outgoing edge, (O, Dn),
    under ONE threshold, that of the bound U sets through O's row."""
    rng = np.random.default_rng(500 + dim + (7 if several else 0))
    n, h = 800, dim // 2
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    sign = rng.choice([-1.0, 1.0], size=dim)
    spots = rng.permutation(n)[:12].tolist()
    O, U, Dn, T, P, Q = spots[:6]
    chain = spots[6:12]
    rows[O] = (np.concatenate([np.full(h, UP), np.full(h, DOWN)]) * sign).astype(np.float32)
    rows[U] = (np.concatenate([np.full(h, UP), np.zeros(h)]) * sign * 2.0).astype(np.float32)
    q = np.concatenate([np.zeros(h), np.full(h, DOWN)])
    q[0] = DOWN * 2.0 ** -4
    rows[Dn] = (q * sign * 0.5).astype(np.float32)
    d1 = rows[U].astype(np.float64) / np.linalg.norm(rows[U].astype(np.float64))
    d2 = rows[Dn].astype(np.float64) / np.linalg.norm(rows[Dn].astype(np.float64))
    d2o = d2 - (d2 @ d1) * d1
    d2o /= np.linalg.norm(d2o)
    e = rng.standard_normal(dim)
    e -= (e @ d1) * d1 + (e @ d2o) * d2o
    e /= np.linalg.norm(e)
    for k, r in zip((1, 2, 3), chain[:3]):  # from Dn to e
        t = np.deg2rad(30.0 * k)
        rows[r] = ((np.cos(t) * d2 + np.sin(t) * e) * rng.uniform(0.5, 2.0)).astype(np.float32)
    for k, r in zip((2, 1), chain[3:5]):  # from e to U
        t = np.deg2rad(30.0 * k)
        rows[r] = ((np.cos(t) * d1 + np.sin(t) * e) * rng.uniform(0.5, 2.0)).astype(np.float32)
    rows[chain[5]] = rng.standard_normal(dim).astype(np.float32)  # (a filler row like the others)
    if several:
        avoid = [rows[U], rows[Dn], e.astype(np.float32)]
        rows[T] = away_from(rng, rows[O], 0.97, avoid)
        rows[P] = away_from(rng, rows[O], 0.93, avoid + [rows[T]])
        rows[Q] = away_from(rng, rows[P], 0.97, avoid + [rows[T], rows[O]])
    rows = np.ascontiguousarray(rows)
    m = margin(dim)
    G, S = cosine_matrix(rows), screen_matrix(rows)
    np.fill_diagonal(G, -1.0)
    np.fill_diagonal(S, -1.0)
    c_up, c_down = oracle.canonical_score(rows[O], rows[U], 0), oracle.canonical_score(rows[O], rows[Dn], 0)
    s_up, s_down = screen_score(rows[O], rows[U]), screen_score(rows[O], rows[Dn])
    print("dim %d: c_up %.6f c_down %.6f s_up %.6f s_down %.6f gap %.5f m %.5f" % (dim, c_up, c_down, s_up, s_down, s_up - s_down, m))
    assert 0.70 < c_up < c_down < 0.72
    assert s_up > c_up + 0.005 and s_down < c_down - 0.005
    assert m + F32_ACC < s_up - s_down < 2 * m - F32_ACC
    mine = [O, T, P, Q] if several else [O]
    other = np.setdiff1d(np.arange(n), mine)
    # U sets the bound of O's component, Dn is its best partner, and nothing else is near: every other foreign row is certainly
    # below the list, and below (O, Dn) in truth
    Sf, Gf = S[np.ix_(mine, other)], G[np.ix_(mine, other)]
    assert Sf.max() == S[O, U] and Gf.max() == G[O, Dn]
    rest = np.ones_like(Sf, dtype=bool)
    rest[mine.index(O), [int(np.nonzero(other == U)[0][0]), int(np.nonzero(other == Dn)[0][0])]] = False
    assert Sf[rest].max() < s_up - 2 * m - F32_ACC and Gf[rest].max() < c_up
    # the tree holds (O, Dn) and the chain and not (O, U) — and Borůvka finds it with a slack of 2 m and not with a slack of m
    tree = kruskal(G)
    key = lambda a, b: (min(a, b), max(a, b))
    assert key(O, Dn) in tree and key(O, U) not in tree
    assert boruvka(G, S, 2 * m) == tree
    assert key(O, U) in boruvka(G, S, m)
    if several:
        assert {key(O, T), key(P, Q), key(O, P)} <= tree
        assert G[O].argmax() == T and G[T].argmax() == O and G[P].argmax() == Q and G[Q].argmax() == P  # round 0: two tight pairs
        pair = [O, T]
        out = np.setdiff1d(np.arange(n), pair)
        Gp = G[np.ix_(pair, out)]
        assert Gp.max() == G[O, P]                                                                        # round 1: they join
    return rows, (O, U, Dn)


@pytest.mark.parametrize("several", [False, True], ids=["one_row", "several_rows"])
@pytest.mark.parametrize("dim", [64, 384])
def test_the_2m_slack(ctx, oracle, dim, several):
    rows, (O, U, Dn) = slack_case(oracle, dim, several)  # (asserts on the CPU before the device is used)
    n = rows.shape[0]
    ids = make_ids(np.random.default_rng(dim), n)
    s = build(ctx, rows, ids)
    got = s.linkage_tree(None)
    st = s.last_linkage_stats()
    print(st)
    check_verified(oracle, rows, ids, got, None, st)
    edges = set(zip(got[2].tolist(), got[3].tolist()))
    assert (min(O, Dn), max(O, Dn)) in edges and (min(O, U), max(O, U)) not in edges
    if several:
        assert st["rounds"] >= 3
    s.close()


# ---- e. the sampled bound pass ----------------------------------------------------------------------------------------------------
def test_sampled_bound_pass_and_partial_last_tile(ctx, oracle):
    """12 320 rows of 64 features are 385 blocks: the bound pass streams every fourth, and the last tile has one block.  Owners in
    the first tile, in one in the middle and in the last one get their best partners (0.999) where the bound pass does not look
    (blocks 5 and 7) and in their own tile: the bound comes from a lesser partner, and the list pass must still find the best."""
    rng = np.random.default_rng(22)
    n, dim = 12320, 64
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    owners = [3, 97, 160 * 32 + 5, 162 * 32 + 31, 384 * 32 + 1, n - 1]
    planted = {}
    for i, r in enumerate(owners):
        own_tile = (r // 128) * 128
        own = own_tile + 40 + i if own_tile + 64 < n else own_tile + 8 + i
        spots = [5 * 32 + 2 * i, 7 * 32 + 2 * i, own]
        assert all(sp != r and (sp // 32) % 4 != 0 for sp in spots[:2]) and own != r and own < n
        for p in spots:
            rows[p] = neighbour(rng, rows[r], 0.999) * np.float32(rng.uniform(0.5, 2.0))
        planted[r] = spots
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    U = rows.astype(np.float64) / np.sqrt(canonical_norm2(rows))[:, None]
    for r, spots in planted.items():  # what is hostile: the planted rows are the owner's best three, and random rows are far below them
        g = U @ U[r]
        g[r] = -1.0
        assert set(np.argsort(-g)[:3].tolist()) == set(spots) and np.sort(g)[-3] > 0.99 and np.sort(g)[-4] < 0.75
    s = build(ctx, rows, ids)
    got = s.linkage_tree(None)
    st = s.last_linkage_stats()
    print(st)
    assert st["tile_rows"] == 128 and st["rows"] == n and st["rounds"] >= 3
    check_verified(oracle, rows, ids, got, None, st)
    edges = set(zip(got[2].tolist(), got[3].tolist()))
    for r, spots in planted.items():  # an owner's best partner is a tree edge (the cut property)
        g = U @ U[r]
        g[r] = -1.0
        b = int(np.argmax(g))
        assert (min(r, b), max(r, b)) in edges
    s.close()


def test_sampled_bound_pass_that_finds_nothing_is_repeated(ctx, oracle):
    """256 blocks of 64-d rows, every fourth block — the sample — of zero rows: no component finds a certified foreign row in the
    sample, though there are 6 143 of them.  Without the repeat at stride 1 every component would list every foreign row: 37 million
    candidates in round 0 instead of a few per row."""
    rng = np.random.default_rng(23)
    n, dim = 8192, 64
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    blocks = np.arange(n) // 32
    rows[blocks % 4 == 0] = 0.0
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    live = takes_part(rows)
    P = int(live.sum())
    assert P == 6144 and not live[blocks % 4 == 0].any() and n // 32 // 64 >= 4  # (the stride: min(4, blocks / 64))
    s = build(ctx, rows, ids)
    got = s.linkage_tree(None)
    st = s.last_linkage_stats()
    print(st)
    check_verified(oracle, rows, ids, got, None, st)
    assert st["reruns"] == 0 and st["candidates"] < 64 * P < P * (P - 1)
    s.close()


# ---- f. equality with the calls that exist ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_cut_equals_density_clusters_and_duplicate_groups(ctx, oracle, metric):
    rng = np.random.default_rng(61)
    n, dim = 600, 96
    centres = rng.standard_normal((8, dim))
    which = rng.integers(0, 8, size=n)
    rows = (centres[which] + rng.uniform(0.3, 1.6, size=(n, 1)) * rng.standard_normal((n, dim))).astype(np.float32)
    spots = rng.permutation(n)[:60]
    for j in range(30):  # copies, scaled copies and close neighbours
        a, b = int(spots[2 * j]), int(spots[2 * j + 1])
        rows[b] = rows[a] if j % 3 == 0 else rows[a] * np.float32(0.5) if j % 3 == 1 else neighbour(rng, rows[a], 0.97)
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(n, 1))).astype(np.float32)
    rows[77] = 0.0
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids, metric, sources=[(1, 0, 333), (2, 333, n)])
    tree = s.linkage_tree(None)
    check(tree, reference(oracle, rows, ids), s.last_linkage_stats())
    t_ids, part, pos_a, pos_b, _ia, _ib, c = tree
    counts = []
    for thr in (0.3, 0.6, 0.9, BELOW_ONE):
        t = float(np.float32(thr))
        labels, clusters = pa.linkage_cut(pos_a, pos_b, c, n, part, t)
        d_ids, d_labels, _kinds, _degrees, d_clusters = s.density_clusters(None, thr, 1)
        np.testing.assert_array_equal(t_ids, d_ids)
        np.testing.assert_array_equal(labels, d_labels)
        assert clusters == d_clusters
        id_a, id_b, _scores, total = s.find_duplicates(None, thr)
        assert total == len(id_a)
        dup_ids, dup_group = pa.duplicate_groups(id_a, id_b)
        groups = {}
        for i, gid in zip(dup_ids.tolist(), dup_group.tolist()):
            groups.setdefault(gid, set()).add(i)
        members = {}
        for i, lab in zip(t_ids.tolist(), labels.tolist()):
            if lab >= 0:
                members.setdefault(lab, set()).add(i)
        assert sorted(sorted(v) for v in members.values() if len(v) > 1) == sorted(sorted(v) for v in groups.values())
        counts.append(clusters)
    print("clusters at 0.3, 0.6, 0.9, below 1:", counts)
    assert counts[0] < counts[1] < counts[2] <= counts[3] and counts[3] < int(part.sum())  # (the copies hold at the f32 below 1)
    P = int(part.sum())
    for K in (1, 2, 10, 50, P):
        labels, clusters = pa.linkage_cut(pos_a, pos_b, c, n, part, min_clusters=K)
        assert clusters == K and len(set(labels[part != 0].tolist())) == K and labels[77] == -1
    s.close()


# ---- g. rows that take no part, wild rows, a view ---------------------------------------------------------------------------------
def test_rows_that_take_no_part_and_wild_rows(ctx, oracle):
    rng = np.random.default_rng(71)
    n, dim = 600, 384
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows[5] = 0.0              # no cosine
    rows[9, 17] = np.nan       # unsearchable
    # |x|^2 beside 2^-126: unit rows a little longer and a little shorter than 1, at 2^-63 of their length
    edge = list(range(200, 212))
    for i, r in enumerate(edge):
        u = rows[r].astype(np.float64)
        rows[r] = (u / np.linalg.norm(u) * (1.0 + (1e-3 if i % 2 else -1e-3)) * 2.0 ** -63).astype(np.float32)
    # wild rows: copies of rows 10.. at |x| about 2^-62 and 2^60 — tree neighbours (cosine 1) the screen cannot certify
    wild = {300: (10, 2.0 ** -66), 301: (11, 2.0 ** 56), 500: (12, 2.0 ** -66), 501: (12, 2.0 ** 56)}
    for r, (src, sc) in wild.items():
        rows[r] = rows[src] * np.float32(sc)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    live = takes_part(rows)
    assert not live[5] and not live[9] and live[edge].sum() == 6 and (~live[edge]).sum() == 6 and live[list(wild)].all()
    n2 = canonical_norm2(rows[list(wild)])
    assert ((n2 < 2.0 ** -40) | (n2 > 2.0 ** 40)).all()
    s = build(ctx, rows, ids)
    got = s.linkage_tree(None)
    want = reference(oracle, rows, ids)
    check(got, want, s.last_linkage_stats())
    np.testing.assert_array_equal(got[1], live.astype(np.int8))
    edges = set(zip(got[2].tolist(), got[3].tolist()))
    assert {(10, 300), (11, 301)} <= edges and len(edges & {(12, 500), (12, 501), (500, 501)}) == 2
    # every pair with a wild row went through the f64 step in round 0
    assert s.last_linkage_stats()["candidates"] >= 2 * len(wild) * (int(live.sum()) - len(wild))
    # hidden rows, a whole block among them
    hidden = [20, 21, 150, 300] + list(range(96, 128))
    s.hide_items(ids[hidden])
    part = np.ones(n, dtype=bool)
    part[hidden] = False
    h = s.linkage_tree(None)
    check(h, reference(oracle, rows, ids, part), s.last_linkage_stats())
    assert (h[1][hidden] == 0).all() and len(h[0]) == n
    s.unhide_items(ids[hidden])
    check(s.linkage_tree(None), want)
    # removed rows: n shrinks and the positions move up
    gone = [0, 33, 599]
    s.remove_items(ids[gone])
    keep = np.setdiff1d(np.arange(n), gone)
    r = s.linkage_tree(None)
    assert len(r[0]) == n - 3
    check(r, reference(oracle, rows[keep], ids[keep]), s.last_linkage_stats())
    # a view equals a fresh searcher of its rows
    allowed = keep[rng.random(len(keep)) < 0.5]
    v = s.view(ids[allowed])
    fresh = build(ctx, rows[allowed], ids[allowed])
    a, b = v.linkage_tree(None), fresh.linkage_tree(None)
    same_bits(a, b)
    check(a, reference(oracle, rows[allowed], ids[allowed]), v.last_linkage_stats())
    assert v.last_linkage_stats()["rows"] == len(allowed)
    v.close()
    fresh.close()
    s.close()


# ---- h. sizes, sources, tile sizes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 31, 33, 129])
def test_few_rows(ctx, oracle, n):
    rng = np.random.default_rng(600 + n)
    dim = 64
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    if n > 2:
        rows[n - 1] = rows[0]                            # the last row (alone in its block or tile) is a copy of the first
        rows[n // 2] = rows[0] * np.float32(3.0)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids)
    got = s.linkage_tree(None)
    st = s.last_linkage_stats()
    check(got, reference(oracle, rows, ids), st)
    assert len(got[6]) == n - 1 and st["rounds"] == (0 if n == 1 else st["rounds"]) and (n > 1 or st["candidates"] == 0)
    # no rows: an empty source list, and a source that does not exist.  n = 0 and nothing is launched
    for sources in ([], [99]):
        empty = s.linkage_tree(sources)
        assert all(len(x) == 0 for x in empty)
        st = s.last_linkage_stats()
        assert st["rows"] == 0 and st["prep_ms"] == 0 and st["tile_rows"] == 0 and st["rounds"] == 0 and st["edges"] == 0
    s.close()


def test_segments_and_source_lists(ctx, oracle):
    rng = np.random.default_rng(81)
    D = 384
    sizes = [64, 96, 32, 1, 128, 5, 300]  # (a piece that is not the last of its source is a whole number of blocks: test_assign_gpu.py)
    src_of = [1, 2, 3, 1, 2, 3, 2]
    n = sum(sizes)
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

    for sources in (None, [3, 1, 2], [2], [3, 1], [1]):
        sel = rows_of([1, 2, 3] if sources is None else sources)
        check(s.linkage_tree(sources), reference(oracle, rows[sel], ids[sel]), s.last_linkage_stats())
    s.close()


@pytest.mark.parametrize("dim,tile", [(64, 128), (576, 128), (640, 64), (1216, 64), (1280, 32)])
def test_tile_sizes(ctx, oracle, dim, tile):
    rng = np.random.default_rng(400 + dim)
    n = 800
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    for j in range(40):  # some structure: pairs at 0.9 across the corpus
        a, b = rng.permutation(n)[:2]
        rows[b] = neighbour(rng, rows[a], 0.9)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids)
    got = s.linkage_tree(None)
    st = s.last_linkage_stats()
    assert st["tile_rows"] == tile
    check_verified(oracle, rows, ids, got, None, st)
    s.close()


# ---- i. list growth ---------------------------------------------------------------------------------------------------------------
def test_list_growth(ctx, oracle):
    """1 024 rows at 0.9995 of one vector beside 1 000 Gaussian rows: each of the 1 024 has every other one within 2 m of its best
    screening score, a million candidates in round 0 for a first room of max(65536, 32 x 2048 launch rows) = 65 536."""
    rng = np.random.default_rng(91)
    near, n, dim = 1024, 2024, 64
    centre = rng.standard_normal(dim).astype(np.float32)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    where = np.sort(rng.permutation(n)[:near])
    for r in where:
        rows[r] = neighbour(rng, centre, 0.9995)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    S = screen_matrix(rows)
    np.fill_diagonal(S, -np.inf)
    surely = (S >= S.max(axis=1, keepdims=True) - 2 * margin(dim) + F32_ACC).sum()
    room = max(65536, 32 * ((n + 31) // 32 * 32))
    print("round 0 surely lists %d candidates, the first room is %d" % (surely, room))
    assert room == 65536 and surely > near * (near - 1) - 1 > 8 * room
    s = build(ctx, rows, ids)
    got = s.linkage_tree(None)
    st = s.last_linkage_stats()
    print(st)
    assert st["reruns"] >= 1 and st["candidates"] >= surely
    check_verified(oracle, rows, ids, got, None, st)
    s.close()


# ---- j. determinism, independence of the search settings, the stats ---------------------------------------------------------------
def test_independent_of_settings_and_repeatable(ctx, oracle):
    rows, ids, sources, _where = chain_corpus(100)
    first = None
    for copy, kernel, flags, cap in (("off", "auto", 0, None), ("int8", "mfma", 32, 64), ("auto", "auto", 0, 4096), ("auto", "wave", 32, None)):
        s = pa.Searcher(ctx, rows.shape[1], "cosine")
        s.set_screening_copy(copy)
        for sid, lo, hi in sources:
            s.add_rows(sid, rows[lo:hi], ids[lo:hi])
        s.finalize()
        s.set_kernel(kernel)
        s.set_tuning(flags)
        if cap:
            s.set_candidate_capacity(cap)
        a = s.linkage_tree(None)
        st_a = s.last_linkage_stats()
        s.search_vectors(None, 5, rows[:3])  # a search in between leaves its pass state behind; the next call does not see it
        b = s.linkage_tree(None)
        st_b = s.last_linkage_stats()
        if first is None:
            check_verified(oracle, rows, ids, a, None, st_a)
            first = a
        same_bits(a, b)
        same_bits(a, first)
        counters = ("rows", "participating", "edges", "candidates", "rounds", "tile_rows", "reruns")
        assert [st_a[k] for k in counters] == [st_b[k] for k in counters]
        assert st_a["edges"] == st_a["participating"] - 1 and st_a["rounds"] >= 1
        assert st_a["prep_ms"] > 0 and st_a["bound_ms"] > 0 and st_a["list_ms"] > 0 and st_a["rescore_ms"] > 0 and st_a["merge_ms"] > 0
        s.close()


# ---- k. argument errors that need the searcher ------------------------------------------------------------------------------------
def test_argument_errors_on_the_device(ctx):
    rng = np.random.default_rng(81)
    n = 40
    s = build(ctx, rng.standard_normal((n, 64)).astype(np.float32), np.arange(n, dtype=np.int64))
    i64 = {k: np.full(n, -77, dtype=np.int64) for k in ("ids", "pos_a", "pos_b", "id_a", "id_b")}
    part = np.full(n, -77, dtype=np.int8)
    c = np.full(n, -77.0, dtype=np.float64)
    rows, edges = C.c_int64(-5), C.c_int64(-5)

    def raw(capacity, arrays=True, ids=True, parts=True, edge_ids=True):
        p = {k: (_ffi.i64p(v) if arrays else None) for k, v in i64.items()}
        return _ffi.lib().pcv_searcher_linkage_tree(
            s._handle, None, 0, capacity, p["ids"] if ids else None, _ffi.i8p(part) if arrays and parts else None, p["pos_a"], p["pos_b"],
            p["id_a"] if edge_ids else None, p["id_b"] if edge_ids else None, _ffi.f64p(c) if arrays else None, C.byref(rows),
            C.byref(edges) if arrays else None)

    assert raw(n) == 0 and rows.value == n and edges.value == n - 1 and (part == 1).all() and (i64["ids"] == np.arange(n)).all()
    assert (i64["pos_a"][: n - 1] < i64["pos_b"][: n - 1]).all() and (np.diff(c[: n - 1]) <= 0).all()
    assert i64["pos_a"][n - 1] == -77 and c[n - 1] == -77.0  # (n - 1 edges: the last slot is not written)
    st = s.last_linkage_stats()
    assert st["rows"] == n and st["edges"] == n - 1 and st["prep_ms"] > 0
    # the count alone: no device work, the stats are zero
    rows.value = -5
    assert raw(0, arrays=False) == 0 and rows.value == n
    st = s.last_linkage_stats()
    assert all(v == 0 for v in st.values()), st
    # capacity < n: PCV_ERR_INVALID with out_rows set and nothing else written
    for v in i64.values():
        v[:] = -77
    rows.value, edges.value = -5, -5
    for cap in (n - 1, 1):
        assert raw(cap) == 1 and rows.value == n and "room for %d rows" % cap in _ffi.lib().pcv_last_error().decode()
        assert (i64["pos_a"] == -77).all() and edges.value == -5
    # out_ids, out_part and the edges' ids may be NULL
    part[:] = -77
    assert raw(n, ids=False, parts=False, edge_ids=False) == 0 and edges.value == n - 1
    assert (i64["ids"] == -77).all() and (part == -77).all() and (i64["id_a"] == -77).all() and (i64["pos_a"][: n - 1] >= 0).all()
    s.set_shard_offset(5)  # a sharded searcher
    with pytest.raises(pa.PcvError) as e:
        s.linkage_tree(None)
    assert e.value.status == 1 and "sharded" in str(e.value)
    s.set_shard_offset(0)
    assert len(s.linkage_tree(None)[6]) == n - 1
    s.add_rows(1, np.ones((1, 64), dtype=np.float32), np.array([99], dtype=np.int64))  # pending rows: as a search
    with pytest.raises(pa.PcvError) as e:
        s.linkage_tree(None)
    assert e.value.status == 1
    s.close()
    wide = build(ctx, np.ones((40, 2560), dtype=np.float32), np.arange(40, dtype=np.int64))
    with pytest.raises(pa.PcvError) as e:
        wide.linkage_tree(None)
    assert e.value.status == 3 and "linkage_tree" in str(e.value)  # PCV_ERR_UNSUPPORTED: rows wider than the tile
    wide.close()


# ---- l. the C++ mirror ------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_linkage_program(oracle, golden_dir, tmp_path):
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
    want = reference(oracle, rows, ids)
    thr = 0.9
    labels, clusters = cut(n, want[1], (want[2], want[3], want[6]), thr)
    assert len(want[6]) == 75 and clusters == 76 - 6 and labels[40] == -1
    raw = tmp_path / "rows.f32"
    rows.astype("<f4").tofile(str(raw))
    args = [str(raw), str(n), str(dim), str(len(want[6])), "%016x" % int(np.array([thr]).view(np.uint64)[0]), str(clusters)]
    for i in range(n):
        args += [str(int(want[1][i])), str(int(labels[i]))]
    for a, b, cc in zip(want[2], want[3], want[6]):
        args += [str(int(a)), str(int(b)), "%016x" % int(np.array([cc]).view(np.uint64)[0])]
    src = os.path.join(ROOT, "tests", "cpp", "linkage_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "linkage_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "linkage_mirror_test: ok" in r.stdout
