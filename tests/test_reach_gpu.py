"""GPU: the reach tree (pcv_searcher_reach_tree), through the Python mirror of the C ABI.  The reference of every check is
reach_ref.py: Kruskal over every participating pair under w = min(core, core, c), c the oracle's canonical cosine and the cores taken
by sorting, for corpora of up to 700 rows; for larger ones the cores from the oracle and the verifier that replays the returned
edges.  Positions, ids, the f64 bits of core, w and c, out_part, the edge count and the stats counters are compared for equality.
Each test first asserts on the CPU what makes its input hostile: ties in w by the hundred, a cap that changes the tree, a
component bound the cap sets with the true edge between one and two margins below it, cores that are no f32, fewer rows than
min_items, rows the screen is not certified for, best partners in blocks the bound pass does not sample."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import linkage_ref
import perceive_amd as pa
import test_linkage_gpu as tl  # its corpora and its CPU models of the screen: the helpers, not the tests
from density_ref import canonical_norm2, margin, takes_part
from duplicates_ref import build, make_ids, neighbour, screen_score
from perceive_amd import _ffi
from reach_ref import bits, check, check_select, check_verified, cores_of, reference, score_matrix, select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

F32_ACC = tl.F32_ACC


def same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def edge_set(t, a=3, b=4):
    return set(zip(t[a].tolist(), t[b].tolist()))


def weights(G, min_items):
    """the weight matrix of a dense cosine matrix G (diagonal ignored) in f64 -> (W, core)"""
    n = G.shape[0]
    H = G.copy()
    np.fill_diagonal(H, -np.inf)
    j = min(min_items - 1, n - 1)
    core = np.full(n, np.inf) if j == 0 else -np.sort(-H, axis=1)[:, j - 1]
    W = np.minimum(G, np.minimum(core[:, None], core[None, :]))
    np.fill_diagonal(W, -1.0)
    return W, core


# ---- a. golden corpora ------------------------------------------------------------------------------------------------------------
_golden = {}


def golden_case(oracle, golden_dir, name, first, metric):
    """rows, ids and the oracle's c of every pair: computed once, shared by the cases of every min_items, never changed"""
    key = (name, metric)
    if key not in _golden:
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        rows = np.array(g["corpus"], dtype=np.float32)[:first]
        rng = np.random.default_rng(21)
        if metric == "dot":  # rows of several lengths: the tree is by cosine all the same
            rows = (rows * rng.uniform(0.5, 1.5, size=(rows.shape[0], 1))).astype(np.float32)
        rows = np.ascontiguousarray(rows)
        ids = make_ids(rng, rows.shape[0])
        _golden[key] = (rows, ids, score_matrix(oracle, rows, list(range(rows.shape[0]))))
    return _golden[key]


@pytest.mark.parametrize("min_items", [1, 2, 5, 16, 65])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("name,first", [("scan_n77_d100", 77), ("scan_n1000_d384", 600)])
def test_golden(ctx, oracle, golden_dir, name, first, metric, min_items):
    rows, ids, G = golden_case(oracle, golden_dir, name, first, metric)
    s = build(ctx, rows, ids, metric)
    got = s.reach_tree(None, min_items)
    st = s.last_reach_stats()
    print(st)
    check(got, reference(oracle, rows, ids, min_items, G=G), st, min_items)
    assert st["tile_rows"] == 128
    s.close()


# ---- b. min_items = 1 is the linkage tree -----------------------------------------------------------------------------------------
def test_min_items_1_equals_linkage_tree(ctx):
    rows, ids, sources, _where = tl.chain_corpus(100)
    s = build(ctx, rows, ids, sources=sources)
    plain = s.linkage_tree(None)
    st_plain = s.last_linkage_stats()
    got = s.reach_tree(None, 1)
    st = s.last_reach_stats()
    ids_, part, core, pos_a, pos_b, id_a, id_b, w, c = got
    same_bits((ids_, part, pos_a, pos_b, id_a, id_b, w), plain)
    same_bits((c,), (plain[6],))
    assert (core == np.inf).all()
    # ... by the same rounds over the same candidates: the cap is +inf everywhere, and the core step is skipped
    assert [st[k] for k in ("rows", "participating", "edges", "candidates", "rounds", "tile_rows")] == [
        st_plain[k] for k in ("rows", "participating", "edges", "candidates", "rounds", "tile_rows")]
    assert st["core_candidates"] == 0 and st["core_ms"] == 0 and st["min_items"] == 1
    s.close()


# ---- c. the cap decides -----------------------------------------------------------------------------------------------------------
def clustered_corpus(metric="cosine"):
    """test_linkage_gpu.py's corpus of the cut test: 600 rows of 96 features around eight centres at several spreads, with copies,
    scaled copies and close neighbours, and a zero row"""
    rng = np.random.default_rng(61)
    n, dim = 600, 96
    centres = rng.standard_normal((8, dim))
    which = rng.integers(0, 8, size=n)
    rows = (centres[which] + rng.uniform(0.3, 1.6, size=(n, 1)) * rng.standard_normal((n, dim))).astype(np.float32)
    spots = rng.permutation(n)[:60]
    for j in range(30):
        a, b = int(spots[2 * j]), int(spots[2 * j + 1])
        rows[b] = rows[a] if j % 3 == 0 else rows[a] * np.float32(0.5) if j % 3 == 1 else neighbour(rng, rows[a], 0.97)
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(n, 1))).astype(np.float32)
    rows[77] = 0.0
    return np.ascontiguousarray(rows), make_ids(rng, n)


def test_the_cap_decides(ctx, oracle):
    rows, ids = clustered_corpus()
    plain = linkage_ref.reference(oracle, rows, ids)
    want = reference(oracle, rows, ids, 5)
    # what is hostile: the two trees differ in their edges, not only in their weights — a screen that forgot the cap, or applied it
    # to the weights alone, returns the wrong tree
    differ = edge_set(want) ^ edge_set(plain, 2, 3)
    print("edges in one tree and not the other: %d" % len(differ))
    assert len(differ) >= 50
    assert (want[7] < want[8]).sum() >= 100 and (want[7] <= want[8]).all()  # the cap, not c, is the weight of many tree edges
    s = build(ctx, rows, ids, sources=[(1, 0, 333), (2, 333, 600)])
    got = s.reach_tree(None, 5)
    check(got, want, s.last_reach_stats(), 5)
    s.close()


# ---- d. mass ties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_items", [4, 17])
def test_ties_identical_rows(ctx, oracle, min_items):
    """Four groups of 16 identical rows over two segments.  min_items = 4: a core is the c of a row with its copies, one value per
    group, and the 120 pairs of a group tie at it.  min_items = 17: a core is a row's best c with ANOTHER group, and whole groups
    of pairs tie below the cap."""
    rng = np.random.default_rng(32)
    dim = 100
    base = rng.standard_normal((4, dim)).astype(np.float32)
    group = rng.permutation(np.repeat(np.arange(4), 16))
    rows = np.ascontiguousarray(base[group])
    ids = make_ids(rng, 64)
    want = reference(oracle, rows, ids, min_items)
    inside = group[want[3]] == group[want[4]]
    w = want[7]
    if min_items == 4:
        assert inside[:60].all() and not inside[60:].any() and (w[:60] > 0.999999).all()
        assert len(set(want[2].tolist())) <= 4
    else:
        assert (want[2] < 0.9).all() and len(set(w.tolist())) <= 4  # 63 edges of at most four weights: the positions order them
    s = build(ctx, rows, ids, sources=[(1, 0, 29), (2, 29, 64)])
    assert s.num_segments == 2
    check(s.reach_tree(None, min_items), want, s.last_reach_stats(), min_items)
    s.close()


@pytest.mark.parametrize("min_items", [3, 65])
def test_ties_the_star(ctx, oracle, min_items):
    rows = np.ascontiguousarray(np.eye(64, dtype=np.float32)[:, ::-1] * np.float32(3.0))
    ids = np.arange(64, dtype=np.int64) * 5 + 2
    G = tl.cosine_matrix(rows)
    assert (G[~np.eye(64, dtype=bool)] == 0.0).all() and (tl.screen_matrix(rows)[~np.eye(64, dtype=bool)] == 0.0).all()
    want = reference(oracle, rows, ids, min_items)
    assert want[3].tolist() == [0] * 63 and want[4].tolist() == list(range(1, 64)) and (want[7] == 0.0).all() and (want[2] == 0.0).all()
    s = build(ctx, rows, ids)
    got = s.reach_tree(None, min_items)
    st = s.last_reach_stats()
    check(got, want, st, min_items)
    assert st["rounds"] == 1 and st["candidates"] == 64 * 63 and st["core_candidates"] == 64 * 63
    s.close()


def test_ties_weights_1e_10_apart(ctx, oracle):
    """test_linkage_gpu.py's families (b, p, p'): p at 0.9 of b, p' = p with one feature moved by an ulp.  At min_items = 2 the core
    of p and p' is their c with each other, nearly 1, and the core of b its best c: w(b, p) = c(b, p) and w(b, p') = c(b, p'),
    about 1e-10 apart, and the family's edge to b is the larger."""
    rng = np.random.default_rng(32)
    dim, n, fam = 100, 600, 100
    rng.standard_normal((4, dim))  # (the draws of the linkage test before its families, so that the corpus is the same)
    rng.permutation(np.repeat(np.arange(4), 16))
    make_ids(rng, 64)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    spots = rng.permutation(n)[: 3 * fam].reshape(fam, 3)
    gaps = []
    for b, p, q in spots:
        rows[p] = neighbour(rng, rows[b], 0.9)
        rows[q] = rows[p]
        effect = np.abs(rows[b].astype(np.float64) - 0.9 * rows[p].astype(np.float64)) * np.spacing(np.abs(rows[p])).astype(np.float64) / float(canonical_norm2(rows[b : b + 1])[0])
        j = int(np.argmin(np.abs(effect - 1e-10)))
        rows[q, j] = np.nextafter(rows[q, j], np.float32(np.inf))
        gaps.append(abs(oracle.canonical_score(rows[b], rows[p], 0) - oracle.canonical_score(rows[b], rows[q], 0)))
    rows = np.ascontiguousarray(rows)
    gaps = np.array(gaps)
    print("gaps %.3g .. %.3g" % (gaps.min(), gaps.max()))
    assert (gaps > 5e-11).all() and (gaps < 2e-10).all()
    ids = make_ids(rng, n)
    want = reference(oracle, rows, ids, 2)
    tree = edge_set(want)
    for b, p, q in spots.tolist():  # the family's edge to b is the one with the larger c, and its w is that c
        cp, cq = oracle.canonical_score(rows[b], rows[p], 0), oracle.canonical_score(rows[b], rows[q], 0)
        better, worse = (p, q) if cp > cq else (q, p)
        assert (min(b, better), max(b, better)) in tree and (min(b, worse), max(b, worse)) not in tree
    s = build(ctx, rows, ids)
    check(s.reach_tree(None, 2), want, s.last_reach_stats(), 2)
    s.close()


# ---- e. the 2 m slack with the cap --------------------------------------------------------------------------------------------------
def boruvka_capped(W, S, klo, khi, slack):
    """test_linkage_gpu.boruvka with the cap, in exact arithmetic: a component's bound is its largest min(S, klo, klo) with a foreign
    row, its candidates are the foreign pairs with S >= bound - slack whose two khi reach bound - slack, and the true weights W
    choose among them.  -> the edges chosen.  It shows what another slack or another rounding would do to an input; it is never an
    expected result."""
    n = W.shape[0]
    comp = np.arange(n)
    edges = set()
    Sc = np.minimum(S, np.minimum(klo[:, None], klo[None, :]))
    while len(set(comp.tolist())) > 1:
        foreign = comp[:, None] != comp[None, :]
        choice = {}
        for root in sorted(set(comp.tolist())):
            mine = comp == root
            bound = np.where(foreign[mine], Sc[mine], -np.inf).max()
            thr = bound - slack
            listed = foreign[mine] & (S[mine] >= thr) & (khi[mine][:, None] >= thr) & (khi[None, :] >= thr)
            Wm = np.where(listed, W[mine], -np.inf)
            best = Wm.max()
            rows_m = np.nonzero(mine)[0]
            pairs = sorted((min(int(rows_m[i]), int(j)), max(int(rows_m[i]), int(j))) for i, j in zip(*np.nonzero(Wm == best)))
            choice[root] = pairs[0]
        before = len(set(comp.tolist()))
        for a, b in choice.values():
            edges.add((a, b))
            ca, cb = comp[a], comp[b]
            if ca != cb:
                comp[comp == max(ca, cb)] = min(ca, cb)
        assert len(set(comp.tolist())) < before
    return edges


def capped_slack_case(oracle, dim):
    """test_linkage_gpu.slack_case's rows O, U, Dn and the chain that joins U and Dn behind O's back: the screen sees c(O, U) 0.0055
    too high and c(O, Dn), O's best outgoing c, 0.0055 too low, and the two screening scores lie between m and 2 m apart.
    Here min_items = 2 and O has a partner T at t = s(O, U) - 0.0015 of it, above both: O and T choose each other in round 0, and
    core(O) = core(T) = t.  From round 1 on the bound of {O, T} is min(s(O, U), klo[O], klo[U]) = klo[O]: the cap sets it, not a
    screening score — and s(O, Dn) lies between one and two margins below the cap.  The best outgoing edge of {O, T} is (O, Dn),
    w = c(O, Dn) (both cores are above it); a slack of m under the capped bound loses it and takes (O, U)."""
    rows, (O, U, Dn) = tl.slack_case(oracle, dim, False)
    n = rows.shape[0]
    m = margin(dim)
    rng = np.random.default_rng(900 + dim)
    s_up, s_down = screen_score(rows[O], rows[U]), screen_score(rows[O], rows[Dn])
    t = s_up - 0.0015
    G0 = tl.cosine_matrix(rows)
    np.fill_diagonal(G0, -1.0)
    quiet = np.nonzero((np.abs(G0[O]) < 0.3) & (np.abs(G0[U]) < 0.3) & (np.abs(G0[Dn]) < 0.3))[0]
    T = int(quiet[np.argmax(G0[quiet].max(axis=1) < 0.62)])  # a filler row, and nobody's best partner by much
    e = rows[Dn].astype(np.float64) - rows[U].astype(np.float64)  # (any third direction to stay away from)
    rows[T] = tl.away_from(rng, rows[O], t, [rows[U], rows[Dn], e.astype(np.float32)])
    rows = np.ascontiguousarray(rows)
    G, S = tl.cosine_matrix(rows), tl.screen_matrix(rows)
    np.fill_diagonal(G, -1.0)
    np.fill_diagonal(S, -1.0)
    W, core = weights(G, 2)
    c_up, c_down = G[O, U], G[O, Dn]
    print("dim %d: t %.6f c_up %.6f c_down %.6f s_up %.6f s_down %.6f m %.5f core O %.6f U %.6f Dn %.6f T %.6f" % (
        dim, G[O, T], c_up, c_down, S[O, U], S[O, Dn], m, core[O], core[U], core[Dn], core[T]))
    # round 0: O and T choose each other
    assert G[O].argmax() == T and G[T].argmax() == O and core[O] == core[T] == G[O, T] and abs(G[O, T] - t) < 1e-6
    assert W[O].argmax() == T and W[T].argmax() == O
    # the cap sets the bound of {O, T}: every certified score of the pair with a foreign row, capped, is at most klo[O], and (O, U) reaches it
    mine, other = [O, T], np.setdiff1d(np.arange(n), [O, T])
    Sc = np.minimum(S, np.minimum(core[:, None], core[None, :]))
    assert S[O, U] > core[O] + 0.001 and core[U] > core[O] and Sc[O, U] == core[O] and Sc[np.ix_(mine, other)].max() == core[O]
    # the true best outgoing edge is (O, Dn), with w = c, and its screening score sits between one and two margins below the cap
    assert W[np.ix_(mine, other)].max() == W[O, Dn] == G[O, Dn] > W[O, U] == G[O, U]
    assert core[O] - 2 * m + F32_ACC < S[O, Dn] < core[O] - m - F32_ACC
    # nothing else of the pair's is near the list
    rest = np.ones((2, len(other)), dtype=bool)
    rest[0, [int(np.nonzero(other == U)[0][0]), int(np.nonzero(other == Dn)[0][0])]] = False
    assert S[np.ix_(mine, other)][rest].max() < core[O] - 2 * m - F32_ACC
    tree = tl.kruskal(W)
    key = lambda a, b: (min(a, b), max(a, b))
    assert key(O, Dn) in tree and key(O, T) in tree and key(O, U) not in tree
    assert boruvka_capped(W, S, core, core, 2 * m) == tree
    wrong = boruvka_capped(W, S, core, core, m)
    assert key(O, U) in wrong and wrong != tree
    return rows, (O, U, Dn, T)


@pytest.mark.parametrize("dim", [64, 384])
def test_the_2m_slack_with_the_cap(ctx, oracle, dim):
    rows, (O, U, Dn, T) = capped_slack_case(oracle, dim)  # (asserts on the CPU before the device is used)
    n = rows.shape[0]
    ids = make_ids(np.random.default_rng(dim), n)
    s = build(ctx, rows, ids)
    got = s.reach_tree(None, 2)
    st = s.last_reach_stats()
    print(st)
    check_verified(oracle, rows, ids, got, 2, None, st)
    edges = edge_set(got)
    assert (min(O, Dn), max(O, Dn)) in edges and (min(O, T), max(O, T)) in edges and (min(O, U), max(O, U)) not in edges
    assert st["rounds"] >= 2
    s.close()


# ---- f. the rounding of the cores ---------------------------------------------------------------------------------------------------
def test_rounding_of_the_cores(ctx, oracle):
    """A row's best edge often has w == core exactly: two rows that are each other's best partner at min_items = 2 have core = c = w.
    The list keeps an edge only if both khi reach the threshold, and the proof allows every threshold up to the component's best
    weight w*: with khi = core rounded UP, khi >= core >= w* >= threshold always; with khi rounded down and a core that is no f32,
    khi < core = w*, and the sharpest threshold the proof allows, w* itself, drops the true edge.  (The device's threshold is a
    margin and more below w*, so its results cannot tell the two roundings apart: the simulation here is what pins the direction,
    and the device must return the tree.)"""
    rng = np.random.default_rng(77)
    n, dim = 300, 64
    rows = np.ascontiguousarray(rng.standard_normal((n, dim)).astype(np.float32))
    ids = make_ids(rng, n)
    G = score_matrix(oracle, rows, list(range(n)))
    want = reference(oracle, rows, ids, 2, G=G)
    core = want[2]
    H = G.copy()
    np.fill_diagonal(H, -np.inf)
    best = H.argmax(axis=1)
    mutual = [a for a in range(n) if best[best[a]] == a and a < best[a]]
    lo = core.astype(np.float32)
    with np.errstate(over="ignore"):
        klo = np.where(lo.astype(np.float64) > core, np.nextafter(lo, np.float32(-np.inf)), lo).astype(np.float64)
        khi = np.where(lo.astype(np.float64) < core, np.nextafter(lo, np.float32(np.inf)), lo).astype(np.float64)
    assert (klo <= core).all() and (core <= khi).all() and (klo < khi).sum() >= n - 2  # nearly no core is an f32
    hostile = [(a, int(best[a])) for a in mutual if klo[a] < core[a]]
    assert len(hostile) >= 20
    tree = edge_set(want)
    for a, b in hostile:
        w = min(core[a], core[b], G[a, b])
        assert w == core[a] == core[b] == G[a, b] and (a, b) in tree  # round 0: w* of {a} is this edge's w
        assert khi[a] >= w and khi[b] >= w                            # rounded up: listed under every threshold up to w*
        assert not (klo[a] >= w) and not (klo[b] >= w)                # rounded down: the threshold w* drops it
    s = build(ctx, rows, ids)
    got = s.reach_tree(None, 2)
    check(got, want, s.last_reach_stats(), 2)
    # ... and the cores the device returns are the f64 values: their float images go either way
    assert ((got[2].astype(np.float32).astype(np.float64) > got[2]).sum() > 50) and ((got[2].astype(np.float32).astype(np.float64) < got[2]).sum() > 50)
    s.close()


# ---- g. small corpora -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 31, 33, 129])
def test_few_rows(ctx, oracle, n):
    """min_items = 5 with fewer than 5 rows: j = P - 1 (0 for one row: +inf)."""
    rng = np.random.default_rng(600 + n)
    dim = 64
    rows = rng.standard_normal((max(n, 1), dim)).astype(np.float32)
    if n > 2:
        rows[n - 1] = rows[0]
        rows[n // 2] = rows[0] * np.float32(3.0)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, max(n, 1))
    s = build(ctx, rows, ids)
    if n == 0:  # no rows: an empty source list, and a source that does not exist.  Nothing is launched
        for sources in ([], [99]):
            empty = s.reach_tree(sources, 5)
            assert all(len(x) == 0 for x in empty)
            st = s.last_reach_stats()
            assert st["rows"] == 0 and st["prep_ms"] == 0 and st["tile_rows"] == 0 and st["rounds"] == 0 and st["edges"] == 0
        s.close()
        return
    want = reference(oracle, rows, ids, 5)
    if n == 1:
        assert want[2].tolist() == [np.inf]
    elif n <= 4:
        assert (want[2] == np.array([min(oracle.canonical_score(rows[a], rows[b], 0) for b in range(n) if b != a) for a in range(n)])).all()
    got = s.reach_tree(None, 5)
    st = s.last_reach_stats()
    check(got, want, st, 5)
    assert len(got[7]) == n - 1 and (n > 1 or (st["candidates"] == 0 and st["core_candidates"] == 0))
    s.close()


# ---- h. the core scores -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_items", [2, 5, 16])
def test_core_scores_and_neighbors(ctx, oracle, min_items):
    rows, ids = clustered_corpus()
    n = rows.shape[0]
    live = np.nonzero(takes_part(rows))[0].tolist()
    G = score_matrix(oracle, rows, live)
    j = min_items - 1
    want = cores_of(G, live, min_items)
    assert np.isnan(want[77]) and np.isfinite(want[live]).all()
    s = build(ctx, rows, ids)
    got = s.reach_tree(None, min_items)
    np.testing.assert_array_equal(bits(got[2]), bits(want))
    _ids, _nbr, scores, counts = s.neighbors(None, j)
    assert (counts[live] == j).all() and counts[77] == 0
    np.testing.assert_array_equal(got[2][live].astype(np.float32).view(np.uint32), scores[live, j - 1].view(np.uint32))
    s.close()


# ---- i. the existing exact DBSCAN -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_items", [2, 5, 16])
def test_cut_equals_density_clusters_on_core_rows(ctx, min_items):
    rows, ids = clustered_corpus()
    n = rows.shape[0]
    s = build(ctx, rows, ids, sources=[(1, 0, 333), (2, 333, n)])
    t_ids, part, core, pos_a, pos_b, _ia, _ib, w, _c = s.reach_tree(None, min_items)
    seen = []
    for thr in (0.3, 0.6, 0.9):
        t = float(np.float32(thr))
        labels, _clusters = pa.linkage_cut(pos_a, pos_b, w, n, part, t)
        d_ids, d_labels, kinds, _degrees, d_clusters = s.density_clusters(None, thr, min_items)
        np.testing.assert_array_equal(t_ids, d_ids)
        is_core = kinds == pa.PCV_DENSITY_CORE
        np.testing.assert_array_equal(is_core, (part != 0) & (core >= t))
        # cluster for cluster: the cut's label and DBSCAN's label name the same sets of core rows
        pairs = set(zip(labels[is_core].tolist(), d_labels[is_core].tolist()))
        assert len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs}) == d_clusters
        # every row with core < t is a singleton of the cut
        low = (part != 0) & ~(core >= t)
        counts = np.bincount(labels[labels >= 0])
        assert (counts[labels[low]] == 1).all()
        seen.append((int(is_core.sum()), int(d_clusters)))
    print("min_items %d: (core rows, clusters) at 0.3, 0.6, 0.9: %s" % (min_items, seen))
    assert seen[0][0] > seen[1][0] > 0 and seen[1][1] > 1  # (the thresholds bite, and core rows are left to cluster)
    s.close()


# ---- j. rows that take no part, wild rows, a view -----------------------------------------------------------------------------------
def test_rows_that_take_no_part_and_wild_rows(ctx, oracle):
    rng = np.random.default_rng(71)
    n, dim, mi = 600, 384, 5
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows[5] = 0.0              # no cosine
    rows[9, 17] = np.nan       # unsearchable
    edge = list(range(200, 212))  # |x|^2 beside 2^-126
    for i, r in enumerate(edge):
        u = rows[r].astype(np.float64)
        rows[r] = (u / np.linalg.norm(u) * (1.0 + (1e-3 if i % 2 else -1e-3)) * 2.0 ** -63).astype(np.float32)
    # wild rows next to their scaled copies: cosine 1 with a row the screen certifies, and cores the screen cannot certify
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
    got = s.reach_tree(None, mi)
    want = reference(oracle, rows, ids, mi)
    check(got, want, s.last_reach_stats(), mi)
    np.testing.assert_array_equal(got[1], live.astype(np.int8))
    assert np.isnan(got[2][~live]).all() and np.isfinite(got[2][live]).all()
    # hidden rows, a whole block among them
    hidden = [20, 21, 150, 300] + list(range(96, 128))
    s.hide_items(ids[hidden])
    part = np.ones(n, dtype=bool)
    part[hidden] = False
    h = s.reach_tree(None, mi)
    check(h, reference(oracle, rows, ids, mi, part), s.last_reach_stats(), mi)
    assert (h[1][hidden] == 0).all() and len(h[0]) == n
    s.unhide_items(ids[hidden])
    check(s.reach_tree(None, mi), want)
    # removed rows: n shrinks and the positions move up
    gone = [0, 33, 599]
    s.remove_items(ids[gone])
    keep = np.setdiff1d(np.arange(n), gone)
    r = s.reach_tree(None, mi)
    assert len(r[0]) == n - 3
    check(r, reference(oracle, rows[keep], ids[keep], mi), s.last_reach_stats(), mi)
    # a view equals a fresh searcher of its rows
    allowed = keep[rng.random(len(keep)) < 0.5]
    v = s.view(ids[allowed])
    fresh = build(ctx, rows[allowed], ids[allowed])
    a, b = v.reach_tree(None, mi), fresh.reach_tree(None, mi)
    same_bits(a, b)
    check(a, reference(oracle, rows[allowed], ids[allowed], mi), v.last_reach_stats(), mi)
    assert v.last_reach_stats()["rows"] == len(allowed)
    v.close()
    fresh.close()
    s.close()


# ---- k. sources, tile sizes, the sampled bound pass ---------------------------------------------------------------------------------
def test_segments_and_source_lists(ctx, oracle):
    rng = np.random.default_rng(81)
    D = 384
    sizes = [64, 96, 32, 1, 128, 5, 300]
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
        check(s.reach_tree(sources, 5), reference(oracle, rows[sel], ids[sel], 5), s.last_reach_stats(), 5)
    s.close()


@pytest.mark.parametrize("dim,tile", [(64, 128), (576, 128), (640, 64), (1216, 64), (1280, 32)])
def test_tile_sizes(ctx, oracle, dim, tile):
    """both sides of each boundary between two tile sizes"""
    rng = np.random.default_rng(400 + dim)
    n = 800
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    for j in range(40):
        a, b = rng.permutation(n)[:2]
        rows[b] = neighbour(rng, rows[a], 0.9)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids)
    got = s.reach_tree(None, 5)
    st = s.last_reach_stats()
    assert st["tile_rows"] == tile
    check_verified(oracle, rows, ids, got, 5, None, st)
    s.close()


def test_sampled_bound_pass_and_partial_last_tile(ctx, oracle):
    """test_linkage_gpu.py's 385 blocks of 64-d rows: the bound passes (the neighbours' and the rounds') stream every fourth block,
    and the owners' best three partners lie in blocks 5 and 7, which they skip, and in the owner's own tile."""
    rng = np.random.default_rng(22)
    n, dim, mi = 12320, 64, 3
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
    for r, spots in planted.items():  # the planted rows are the owner's best three: its core (the second best) is one of theirs
        g = U @ U[r]
        g[r] = -1.0
        assert set(np.argsort(-g)[:3].tolist()) == set(spots) and np.sort(g)[-3] > 0.99 and np.sort(g)[-4] < 0.75
    s = build(ctx, rows, ids)
    got = s.reach_tree(None, mi)
    st = s.last_reach_stats()
    print(st)
    assert st["tile_rows"] == 128 and st["rows"] == n and st["rounds"] >= 3
    check_verified(oracle, rows, ids, got, mi, None, st)
    for r in planted:
        assert got[2][r] > 0.99
    s.close()


# ---- l. determinism, independence of the search settings ----------------------------------------------------------------------------
def test_independent_of_settings_and_repeatable(ctx, oracle):
    rows, ids, sources, _where = tl.chain_corpus(100)
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
        a = s.reach_tree(None, 5)
        st_a = s.last_reach_stats()
        s.search_vectors(None, 5, rows[:3])  # a search in between leaves its pass state behind; the next call does not see it
        b = s.reach_tree(None, 5)
        st_b = s.last_reach_stats()
        if first is None:
            check_verified(oracle, rows, ids, a, 5, None, st_a)
            first = a
        same_bits(a, b)
        same_bits(a, first)
        counters = ("rows", "participating", "edges", "core_candidates", "candidates", "rounds", "tile_rows", "reruns", "min_items")
        assert [st_a[k] for k in counters] == [st_b[k] for k in counters]
        P = st_a["participating"]
        assert st_a["edges"] == P - 1 and 1 <= st_a["rounds"] <= int(np.ceil(np.log2(P)))
        assert all(st_a[k] > 0 for k in ("core_ms", "prep_ms", "bound_ms", "list_ms", "rescore_ms", "merge_ms"))
        s.close()


# ---- m. argument errors that need the searcher --------------------------------------------------------------------------------------
def test_argument_errors_on_the_device(ctx):
    rng = np.random.default_rng(81)
    n = 40
    s = build(ctx, rng.standard_normal((n, 64)).astype(np.float32), np.arange(n, dtype=np.int64))
    i64 = {k: np.full(n, -77, dtype=np.int64) for k in ("ids", "pos_a", "pos_b", "id_a", "id_b")}
    f64 = {k: np.full(n, -77.0, dtype=np.float64) for k in ("core", "w", "c")}
    part = np.full(n, -77, dtype=np.int8)
    rows, edges = C.c_int64(-5), C.c_int64(-5)

    def raw(capacity, arrays=True, optional=True):
        p = {k: (_ffi.i64p(v) if arrays else None) for k, v in i64.items()}
        q = {k: (_ffi.f64p(v) if arrays else None) for k, v in f64.items()}
        opt = arrays and optional
        return _ffi.lib().pcv_searcher_reach_tree(
            s._handle, None, 0, 5, capacity, p["ids"] if opt else None, _ffi.i8p(part) if opt else None, q["core"] if opt else None, p["pos_a"],
            p["pos_b"], p["id_a"] if opt else None, p["id_b"] if opt else None, q["w"], q["c"] if opt else None, C.byref(rows),
            C.byref(edges) if arrays else None)

    assert raw(n) == 0 and rows.value == n and edges.value == n - 1 and (part == 1).all() and (i64["ids"] == np.arange(n)).all()
    assert (i64["pos_a"][: n - 1] < i64["pos_b"][: n - 1]).all() and (np.diff(f64["w"][: n - 1]) <= 0).all()
    assert (f64["w"][: n - 1] <= f64["c"][: n - 1]).all() and (f64["core"] > -1).all()
    assert i64["pos_a"][n - 1] == -77 and f64["w"][n - 1] == -77.0  # (n - 1 edges: the last slot is not written)
    st = s.last_reach_stats()
    assert st["rows"] == n and st["edges"] == n - 1 and st["prep_ms"] > 0 and st["min_items"] == 5
    # the count alone: no device work, the stats are zero
    rows.value = -5
    assert raw(0, arrays=False) == 0 and rows.value == n
    st = s.last_reach_stats()
    assert all(v == 0 for v in st.values()), st
    # capacity < n: PCV_ERR_INVALID with out_rows set and nothing else written
    for v in i64.values():
        v[:] = -77
    rows.value, edges.value = -5, -5
    for cap in (n - 1, 1):
        assert raw(cap) == 1 and rows.value == n and "room for %d rows" % cap in _ffi.lib().pcv_last_error().decode()
        assert (i64["pos_a"] == -77).all() and edges.value == -5
    # out_ids, out_part, out_core, out_c and the edges' ids may be NULL
    part[:] = -77
    f64["core"][:] = -77.0
    f64["c"][:] = -77.0
    assert raw(n, optional=False) == 0 and edges.value == n - 1
    assert (i64["ids"] == -77).all() and (part == -77).all() and (i64["id_a"] == -77).all() and (i64["pos_a"][: n - 1] >= 0).all()
    assert (f64["core"] == -77.0).all() and (f64["c"] == -77.0).all()
    with pytest.raises(pa.PcvError) as e:  # min_items out of range, through the mirror
        s.reach_tree(None, 66)
    assert e.value.status == 1 and "min_items" in str(e.value)
    s.set_shard_offset(5)  # a sharded searcher
    with pytest.raises(pa.PcvError) as e:
        s.reach_tree(None, 5)
    assert e.value.status == 1 and "sharded" in str(e.value)
    s.set_shard_offset(0)
    assert len(s.reach_tree(None, 5)[7]) == n - 1
    s.add_rows(1, np.ones((1, 64), dtype=np.float32), np.array([99], dtype=np.int64))  # pending rows: as a search
    with pytest.raises(pa.PcvError) as e:
        s.reach_tree(None, 5)
    assert e.value.status == 1
    s.close()
    wide = build(ctx, np.ones((40, 2560), dtype=np.float32), np.arange(40, dtype=np.int64))
    with pytest.raises(pa.PcvError) as e:
        wide.reach_tree(None, 5)
    assert e.value.status == 3 and "reach_tree" in str(e.value)  # PCV_ERR_UNSUPPORTED: rows wider than the tile
    assert wide.search_vectors(None, 3, np.ones((1, 2560), dtype=np.float32))[0].shape == (1, 3)  # ... and the searcher is still usable
    wide.close()


# ---- n. end to end: topics without a threshold --------------------------------------------------------------------------------------
def topic_corpus(n=2000, topics=8, topic_rows=100, seed=11):
    """tools/bench_density.py's corpus at a small size: `topics` centres with `topic_rows` rows each at cosine about 0.9 of their
    centre, shuffled among Gaussian filler"""
    D = 384
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((topics, D))
    centres /= np.linalg.norm(centres, axis=1)[:, None]
    topic_of = np.full(n, -1, dtype=np.int64)
    topic_of[rng.permutation(n)[: topics * topic_rows]] = np.repeat(np.arange(topics), topic_rows)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    member = topic_of >= 0
    rows[member] = (0.9 * centres[topic_of[member]] + np.sqrt(0.19 / D) * rows[member]).astype(np.float32)
    return np.ascontiguousarray(rows), topic_of


def prim_tree(W):
    """a maximum spanning tree of a dense weight matrix by Prim, edges ordered by (w descending, a, b): the CPU's own tree, good for
    counting clusters (ties may fall otherwise than in the edge order; it is never compared with the device's)"""
    n = W.shape[0]
    inside = np.zeros(n, dtype=bool)
    inside[0] = True
    best, frm = W[0].copy(), np.zeros(n, dtype=np.int64)
    best[0] = -np.inf
    edges = []
    for _ in range(n - 1):
        v = int(np.argmax(best))
        edges.append((min(v, int(frm[v])), max(v, int(frm[v])), float(best[v])))
        inside[v] = True
        best[v] = -np.inf
        better = ~inside & (W[v] > best)
        best[better], frm[better] = W[v][better], v
    edges.sort(key=lambda e: (-e[2], e[0], e[1]))
    return (np.array([e[0] for e in edges]), np.array([e[1] for e in edges]), np.array([e[2] for e in edges]))


def test_end_to_end_topics(ctx, oracle):
    rows, topic_of = topic_corpus()
    n, topics = rows.shape[0], int(topic_of.max()) + 1
    ids = np.arange(n, dtype=np.int64)
    # on the CPU alone: the f64 weights, a spanning tree of them, the selection — one cluster per planted topic, each topic whole in
    # its own.  (A filler row that hangs on a topic's subtree below the topic's birth leaves that cluster and so carries its label: a
    # few do, the rest is noise.)
    W, _core = weights(tl.cosine_matrix(rows), 8)
    labels, stab, size = select(n, None, prim_tree(W), 20)
    assert len(stab) == topics
    for t in range(topics):
        assert len(set(labels[topic_of == t].tolist())) == 1 and labels[topic_of == t][0] >= 0
    assert len({int(labels[topic_of == t][0]) for t in range(topics)}) == topics
    print("filler rows with a label: %d of %d; sizes %s" % ((labels[topic_of < 0] >= 0).sum(), (topic_of < 0).sum(), size.tolist()))
    assert (size >= 100).all() and (labels[topic_of < 0] == -1).sum() > (labels[topic_of < 0] >= 0).sum()
    # the device: the tree is the definition's (the cores from the oracle, the tree by the verifier), and the library's selection on it
    # is the plain Python's, label for label — which is the CPU's
    s = build(ctx, rows, ids)
    got = s.reach_tree(None, 8)
    st = s.last_reach_stats()
    print(st)
    check_verified(oracle, rows, ids, got, 8, None, st)
    sel = pa.linkage_select(got[3], got[4], got[7], n, got[1], 20)
    check_select(sel, select(n, got[1], (got[3], got[4], got[7]), 20))
    assert len(sel[1]) == topics
    for t in range(topics):
        assert len(set(sel[0][topic_of == t].tolist())) == 1 and sel[0][topic_of == t][0] >= 0
    s.close()


# ---- o. the C++ mirror ------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_reach_program(oracle, golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "scan_n77_d100.npz"))
    rows = np.array(g["corpus"], dtype=np.float32)
    rng = np.random.default_rng(91)
    for base, others in ((4, (20, 33, 64, 65, 66, 70)), (10, (11, 76, 30, 31, 32)), (50, (51,))):
        for r in others:
            rows[r] = neighbour(rng, rows[base], 0.97)
    rows[40] = 0.0
    rows = np.ascontiguousarray(rows)
    n, dim = rows.shape
    ids = 5000 + 3 * np.arange(n, dtype=np.int64)
    mi, M = 5, 5
    want = reference(oracle, rows, ids, mi)
    labels, stab, size = select(n, want[1], (want[3], want[4], want[7]), M)
    print("clusters", size.tolist())
    fam_a, fam_b = [4, 20, 33, 64, 65, 66, 70], [10, 11, 76, 30, 31, 32]
    assert len(want[7]) == 75 and len(stab) == 2 and labels[40] == -1  # the two planted families of seven and six rows, each a cluster
    assert len(set(labels[fam_a].tolist())) == 1 and len(set(labels[fam_b].tolist())) == 1 and 0 <= labels[4] != labels[10] >= 0
    raw = tmp_path / "rows.f32"
    rows.astype("<f4").tofile(str(raw))
    hexbits = lambda x: "%016x" % int(np.array([x], dtype=np.float64).view(np.uint64)[0])
    args = [str(raw), str(n), str(dim), str(mi), str(len(want[7])), str(M), str(len(stab))]
    for i in range(n):
        args += [str(int(want[1][i])), hexbits(want[2][i]), str(int(labels[i]))]
    for a, b, w, c in zip(want[3], want[4], want[7], want[8]):
        args += [str(int(a)), str(int(b)), hexbits(w), hexbits(c)]
    for sv, sz in zip(stab, size):
        args += [hexbits(sv), str(int(sz))]
    src = os.path.join(ROOT, "tests", "cpp", "reach_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "reach_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "reach_mirror_test: ok" in r.stdout
