"""The reference of compound queries (pcv_searcher_search_compound), in Python and float64, written from the definition in
include/perceive_hip.h and independent of the library: oracle.topk over all rows gives each vector's whole ranked list and with it
every row's canonical score under that vector (as boost_ref.BoostReference obtains its lists); relevance, the min / max, the hinge and
the difference are np.float64 scalars, one operation per line; `walk` grows the examined prefixes in steps of 128, takes the union of
the steps' entries, drops the repeats, and tests the STRICT certificate and the end of a list after each step; `brute` sorts all rows
under m.  The shared corpus of the CPU and GPU tests (the planted corpus of test_distinct_gpu.py plus bridge rows) is built here too."""
import numpy as np

STEP = 128  # PCV_MAX_RESULTS
MAX_PARTS = 8  # PCV_MAX_COMPOUND_PARTS
MAX_POOL = 4096  # PCV_MAX_COMPOUND_POOL
ALL, ANY = 0, 1  # PCV_COMPOUND_ALL, PCV_COMPOUND_ANY
F64 = np.float64


def default_pool(k):
    return min(MAX_POOL, max(128, 8 * k))


def reported(c, metric, dim):
    """what pcv_searcher_search reports for a canonical score: (float)c for cosine, max(0, 1 - c / dim) in f64 then f32 for dot"""
    c = np.asarray(c, dtype=np.float64)
    if metric == "dot":
        d = 1.0 - c / np.float64(dim)
        return np.where(d > 0.0, d, 0.0).astype(np.float32)
    return c.astype(np.float32)


def relevance(c, metric, dim):
    c = F64(c)
    if metric == "dot":
        return c / F64(dim)
    return c


def combine(rel_want, rel_avoid, mode, lam):
    """rel_want, rel_avoid: lists of np.float64 -> (m, pen); lam: the f32 avoid_weight, widened"""
    base = rel_want[0]
    for r in rel_want[1:]:
        if mode == ALL:
            base = r if r < base else base
        else:
            base = r if r > base else base
    hinge = F64(0.0)
    for r in rel_avoid:
        hinge = r if r > hinge else hinge
    pen = F64(np.float32(lam)) * hinge
    m = base - pen
    return m, pen


def order(m, rows):
    """rows sorted by (m descending, position ascending)"""
    return sorted(rows, key=lambda x: (-float(m[x]), x))


def walk_lists(lists, rel_last, m, k, pool, mode):
    """lists[j]: the ranked positions of wanted vector j, best first; rel_last(j, r): the relevance of entry r of list j; m: {position:
    np.float64} for every row with a defined score under all the compound's vectors (others are no candidates).
    -> (kept positions best first, examined, exact)"""
    kept, examined = [], 0
    while True:
        ask = min(STEP, pool - examined)
        got = [min(ask, len(L) - examined) for L in lists]
        got = [max(g, 0) for g in got]
        cands = []
        for L, g in zip(lists, got):  # candidate index: list by list, entry by entry
            cands += list(L[examined:examined + g])
        fresh, before, held = [], set(), set(kept)
        for x in cands:
            repeat = x in held or x in before  # already kept, or at a lower candidate index in this step
            before.add(x)
            if not repeat and x in m:
                fresh.append(x)
        kept = order(m, kept + fresh)[:k]
        most = max(got)
        if min(got) < ask:  # a list ended: every selectable row has been met
            return kept, examined + most, True
        examined += most
        lasts = [rel_last(j, examined - 1) for j in range(len(lists))]
        T = min(lasts) if mode == ALL else max(lasts)
        if len(kept) == k and m[kept[-1]] > T:  # strictly: an unmet row with m == T may have the lower position
            return kept, examined, True
        if examined == pool:
            return kept, examined, False


class Walk:
    """pos, ids, combined (f64), parts (reported f32 [n, MAX_PARTS], NaN behind W), penalties (f64), examined, exact"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class CompoundReference:
    """vectors [V, dim]: every vector the tests use, wanted or avoided; a compound names them by index."""

    def __init__(self, oracle, vectors, rows, ids, metric):
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.ids, self.metric, self.dim = np.asarray(ids, dtype=np.int64), metric, self.rows.shape[1]
        n = self.rows.shape[0]
        self.pos, self.sc, self.cnt = oracle.topk(vectors, self.rows, n, metric=1 if metric == "dot" else 0)
        self.score = np.full((len(vectors), n), np.nan, dtype=np.float64)  # canonical score of every listed row under every vector
        for v in range(len(vectors)):
            c = int(self.cnt[v])
            self.score[v, self.pos[v, :c]] = self.sc[v, :c]
        self.cache = {}

    def ranked(self, v, allowed=None):
        c = int(self.cnt[v])
        L = self.pos[v, :c]
        if allowed is not None:
            L = L[np.isin(L, allowed)]
        return L

    def _m(self, want, avoid, mode, lam, allowed):
        vs = list(want) + list(avoid)
        ok = ~np.isnan(self.score[vs]).any(axis=0)
        if allowed is not None:
            ok &= np.isin(np.arange(ok.size), allowed)
        m, pen = {}, {}
        for x in np.nonzero(ok)[0].tolist():
            rw = [relevance(self.score[v, x], self.metric, self.dim) for v in want]
            ra = [relevance(self.score[v, x], self.metric, self.dim) for v in avoid]
            m[x], pen[x] = combine(rw, ra, mode, lam)
        return m, pen

    def _result(self, want, kept, m, pen, examined, exact):
        parts = np.full((len(kept), MAX_PARTS), np.nan, dtype=np.float32)
        for j, v in enumerate(want):
            parts[:, j] = reported(self.score[v, kept], self.metric, self.dim) if kept else []
        return Walk(pos=np.array(kept, dtype=np.int64), ids=self.ids[kept] if kept else np.zeros(0, np.int64),
                    combined=np.array([m[x] for x in kept], dtype=np.float64), parts=parts,
                    penalties=np.array([pen[x] for x in kept], dtype=np.float64), examined=examined, exact=bool(exact))

    def _scored(self, want, avoid, mode, lam, allowed):
        key = (tuple(want), tuple(avoid), mode, float(np.float32(lam)), None if allowed is None else np.asarray(allowed).tobytes())
        if key not in self.cache:
            self.cache[key] = self._m(want, avoid, mode, lam, allowed)
        return self.cache[key]

    def walk(self, want, avoid, mode, lam, k, pool, allowed=None):
        m, pen = self._scored(want, avoid, mode, lam, allowed)
        lists = [self.ranked(v, allowed).tolist() for v in want]

        def rel_last(j, r):
            return relevance(self.score[want[j], lists[j][r]], self.metric, self.dim)

        kept, examined, exact = walk_lists(lists, rel_last, m, k, pool, mode)
        return self._result(want, kept, m, pen, examined, exact)

    def brute(self, want, avoid, mode, lam, k, allowed=None):
        m, pen = self._scored(want, avoid, mode, lam, allowed)
        kept = order(m, list(m.keys()))[:k]
        return self._result(want, kept, m, pen, None, True)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(got, want, i, k, rows_only=False):
    """got: what Searcher.search_compound returned; want: a Walk of compound i.  Ids, counts, examined and exact for equality,
    combined scores and penalties by their 64 bits, part scores by their 32 bits, and the fill values behind the kept rows."""
    ids, combined, parts, penalties, counts, examined, exact = got
    n = len(want.pos)
    print("compound %d: kept %d/%d examined %d/%s exact %s/%s" % (i, int(counts[i]), n, int(examined[i]), want.examined, bool(exact[i]), want.exact))
    assert ids.shape == (len(counts), k) and combined.shape == ids.shape and penalties.shape == ids.shape and parts.shape == (len(counts), k, MAX_PARTS)
    assert int(counts[i]) == n, (i, int(counts[i]), n)
    np.testing.assert_array_equal(ids[i, :n], want.ids)
    np.testing.assert_array_equal(bits64(combined[i, :n]), bits64(want.combined))
    np.testing.assert_array_equal(bits64(penalties[i, :n]), bits64(want.penalties))
    w = int((~np.isnan(want.parts[0])).sum()) if n else 0
    np.testing.assert_array_equal(bits32(parts[i, :n, :w]), bits32(want.parts[:, :w]))
    assert np.isnan(parts[i, :n, w:]).all()
    assert (ids[i, n:] == -1).all() and np.isnan(combined[i, n:]).all() and np.isnan(penalties[i, n:]).all() and np.isnan(parts[i, n:]).all()
    if not rows_only:
        assert int(examined[i]) == want.examined, (i, int(examined[i]), want.examined)
        assert bool(exact[i]) == want.exact, i


# ---- the corpus and the compounds the CPU and GPU tests share ---------------------------------------------------------------------
BRIDGES = ((0, 1), (2, 3), (4, 5), (6, 7), (0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 2, 3, 4, 5, 6, 7))
BRIDGE_ROWS, BRIDGE_COS = 12, 0.98


def bridged_corpus(planted_corpus, metric, dim=384, seed=23):
    """planted_corpus(metric, dim) of test_distinct_gpu.py plus, for every tuple of anchors in BRIDGES, a family of BRIDGE_ROWS rows
    at cosine BRIDGE_COS of the normalised sum of the anchors' unit vectors — rows close to ALL of them, which no family of a single
    anchor is; the rows shuffled again so that the bridges lie in every segment.  -> (rows, ids, anchors, bridge ids per tuple)"""
    rows, ids, anchors = planted_corpus(metric, dim=dim)
    rng = np.random.default_rng(seed)
    groups, bridge_ids = [], []
    next_id = int(ids.max()) + 1000
    for tup in BRIDGES:
        u = sum(anchors[a] / np.linalg.norm(anchors[a]) for a in tup)
        u = u / np.linalg.norm(u)
        noise = rng.standard_normal((BRIDGE_ROWS, dim))
        noise -= np.outer(noise @ u, u)
        noise /= np.linalg.norm(noise, axis=1, keepdims=True)
        fam = np.sqrt(dim) * (BRIDGE_COS * u + np.sqrt(1 - BRIDGE_COS ** 2) * noise)
        if metric == "dot":
            fam = fam * rng.uniform(0.5, 1.5, size=(BRIDGE_ROWS, 1))
        groups.append(fam.astype(np.float32))
        bridge_ids.append(np.arange(next_id, next_id + 3 * BRIDGE_ROWS, 3, dtype=np.int64))
        next_id += 100
    rows = np.concatenate([rows] + groups)
    ids = np.concatenate([ids] + bridge_ids)
    perm = rng.permutation(rows.shape[0])
    return np.ascontiguousarray(rows[perm]), ids[perm], anchors, bridge_ids


def compound_vectors(planted_queries, metric, anchors, dim=384, seed=31):
    """vectors 0..7: noisy anchors, 8..15: Gaussian rows (planted_queries of test_distinct_gpu.py), 16..23: eight more Gaussian
    rows (what the avoided sides draw from)"""
    q = planted_queries(metric, anchors, dim)
    extra = np.random.default_rng(seed).standard_normal((8, dim)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([q, extra]), dtype=np.float32)


# (wanted vector indices, avoided vector indices): W in {1, 2, 4, 8}, A in {0, 1, 8}
COMPOUNDS = [
    ((0,), ()),                                   # W = 1: the plain list
    ((0, 1), ()),                                 # a pair of planted neighbours: the bridge family answers ALL
    ((2, 3), (0,)),                               # ... with an avoided vector that has nothing to do with them
    ((4, 5), (4,)),                               # ... and one that is a wanted vector: every good row pays
    ((8, 9), ()),                                 # a pair of Gaussian queries: nothing stands out
    ((10, 11), (16, 17, 18, 19, 20, 21, 22, 23)),  # A = 8
    ((0, 1, 2, 3), ()),                           # W = 4
    ((4, 5, 6, 7), (12,)),
    ((8, 9, 10, 11), (16, 17, 18, 19, 20, 21, 22, 23)),
]
COMPOUNDS_W8 = [
    ((0, 1, 2, 3, 4, 5, 6, 7), ()),               # W = 8 (the MFMA forms)
    ((8, 9, 10, 11, 12, 13, 14, 15), (0,)),
    ((0, 1, 2, 3, 4, 5, 6, 7), (16, 17, 18, 19, 20, 21, 22, 23)),
]
LAMBDAS = (0.0, 0.5, 4.0)
CASES = [(k, pool) for k in (1, 10, 128) for pool in sorted({k, 128, 129, 300, MAX_POOL}) if pool >= k]
