"""The reference of the diverse-results tests (pcv_searcher_search_diverse; include/perceive_hip.h states the definition).

Per query, oracle.topk over all rows gives the ranked list L; the greedy walk below runs over its first `pool` entries in Python
floats (IEEE f64, no fused multiply-add: the three roundings of the marginal value are three statements), with
orc_canonical_score(row, row, dim, 0) as the pair cosine, remembered per corpus.  walk(..., pool=None) is the same walk over all
of L: what the certificate out_exact promises."""
import ctypes as C

import numpy as np

_FP = C.POINTER(C.c_float)
D0 = 1.0 + 2.0 ** -40  # no canonical cosine falls below -D0
N_ANCHOR = 8
FAMILIES = ((0.999, 20), (0.99, 20), (0.97, 20), (0.9, 12))
SPLIT = (400, 2000)  # source 1: rows [0, 400) and [400, 2000) in two segments; source 2: the rest


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def reported(c, metric, dim):
    """hits_to_outputs: (float)c for cosine, max(0, 1 - c / dim) in f64 then f32 for the dot metric"""
    c = np.asarray(c, dtype=np.float64)
    if metric == "dot":
        d = 1.0 - c / np.float64(dim)
        return np.where(d > 0.0, d, 0.0).astype(np.float32)
    return c.astype(np.float32)


def default_pool(k):
    return min(4096, max(128, 8 * k))


def planted_corpus(metric, dim=384, seed=5, n_base=2600, families=FAMILIES, n_anchor=N_ANCHOR):
    """Gaussian rows plus, per anchor row, families at a given cosine of it; rows shuffled, ids permuted and not contiguous; for
    the dot metric every row times an amplitude of its own in [0.5, 1.5)"""
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


class Walk:
    """What one walk came to: ranks (in L, pick order), rows (positions in the corpus), ids, scores (reported f32), marginal (f64),
    examined (|P|), exact (the certificate as perceive_hip.h defines it), bound (the certificate's bound; None for an empty pool),
    rel_last"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Reference:
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
        """canonical cosine of rows a and b (symmetric bit for bit; asked with the lower row first); a pair without one counts as 0"""
        key = (a, b) if a <= b else (b, a)
        c = self.pairs.get(key)
        if c is None:
            c = self.lib.orc_canonical_score(self.ptr[key[0]], self.ptr[key[1]], self.dim, 0)
            if c != c:
                c = 0.0
            self.pairs[key] = c
        return c

    def rel(self, c):
        return c / float(self.dim) if self.metric == "dot" else c

    def ranked(self, q, allowed=None):
        n = int(self.cnt[q])
        L, sc = self.pos[q, :n], self.sc[q, :n]
        if allowed is not None:
            ok = np.isin(L, allowed)
            L, sc = L[ok], sc[ok]
        return L.tolist(), sc.tolist()

    def walk(self, q, k, lam, pool, allowed=None):
        """pool=None: over all of L"""
        lam = float(np.float32(lam))  # (double)lambda
        key = (q, k, lam, pool, None if allowed is None else allowed.tobytes())
        if key in self.walks:
            return self.walks[key]
        L, sc = self.ranked(q, allowed)
        P = L if pool is None else L[:pool]
        n = len(P)
        mu = 1.0 - lam
        rel = [self.rel(c) for c in sc[:n]]
        div = [0.0] * n
        free = list(range(n))
        ranks, marginal = [], []
        while free and len(ranks) < k:
            best, best_m = -1, None
            for i in free:  # ascending rank: a strict comparison breaks ties to the lower rank
                a = lam * rel[i]
                b = mu * div[i]
                m = a - b
                if best_m is None or m > best_m:
                    best, best_m = i, m
            first = not ranks
            ranks.append(best)
            marginal.append(best_m)
            free.remove(best)
            if mu != 0.0 and len(ranks) < k:  # (mu == 0: b is a zero whatever div is)
                row = P[best]
                for i in free:
                    c = self.cos(P[i], row)
                    if first or c > div[i]:
                        div[i] = c
        bound, rel_last = None, None
        exact = pool is None or n < pool
        if n:
            rel_last = rel[n - 1]
            a = lam * rel_last
            b = mu * D0
            bound = a + b
            exact = exact or all(m > bound for m in marginal)
        rows = [P[i] for i in ranks]
        out = Walk(ranks=np.array(ranks, dtype=np.int32), rows=rows, ids=self.ids[rows] if rows else np.zeros(0, np.int64),
                   scores=reported([sc[i] for i in ranks], self.metric, self.dim), marginal=np.array(marginal, dtype=np.float64),
                   examined=n, exact=bool(exact), bound=bound, rel_last=rel_last, lam=lam, mu=mu)
        self.walks[key] = out
        return out


def check(got, want, q, k):
    """got: what Searcher.search_diverse returned; want: a Walk.  Everything is compared for equality (scores as f32 bits, marginal
    as f64 bits), and the fill values behind the picks"""
    ids, scores, marginal, ranks, counts, examined, exact = got
    n = len(want.ranks)
    print("query %d: picks %d/%d examined %d/%d exact %s/%s last rank %s" % (
        q, int(counts[q]), n, int(examined[q]), want.examined, bool(exact[q]), want.exact, want.ranks[-1] if n else None))
    assert ids.shape == (len(counts), k) and scores.shape == ids.shape and marginal.shape == ids.shape and ranks.shape == ids.shape
    assert int(counts[q]) == n, (q, int(counts[q]), n)
    np.testing.assert_array_equal(ranks[q, :n], want.ranks)
    np.testing.assert_array_equal(ids[q, :n], want.ids)
    np.testing.assert_array_equal(bits32(scores[q, :n]), bits32(want.scores))
    np.testing.assert_array_equal(bits64(marginal[q, :n]), bits64(want.marginal))
    assert int(examined[q]) == want.examined, (q, int(examined[q]), want.examined)
    assert bool(exact[q]) == want.exact, (q, bool(exact[q]), want.exact)
    assert (ids[q, n:] == -1).all() and np.isnan(scores[q, n:]).all() and np.isnan(marginal[q, n:]).all() and (ranks[q, n:] == -1).all()
