"""The reference of boosted search (pcv_searcher_search_boosted), in Python and float64, written from the definition in
include/perceive_hip.h: the ranked list L of a query comes from oracle.topk over all rows (as where_ref.WhereReference obtains it),
the boost is evaluated with Python ints and np.float64 scalars, one operation per line, the walk grows the examined prefix in steps
of 128 and tests the certificate after each, and a brute-force top-k over all of L by (m, rank) stands beside it."""
import numpy as np

from grouped_ref import default_pool, reported  # noqa: F401  (the Python default of `pool` is grouped_ref's rule)

NO_VALUE = -(1 << 63)
STEP = 128  # PCV_MAX_RESULTS
MAX_KNOTS = 16
MAX_POOL = 4096
F64 = np.float64


class Boost:
    """knot_values (Python ints, strictly increasing), knot_boosts and unset_boost (np.float64)"""

    def __init__(self, knot_values, knot_boosts, unset_boost=0.0):
        self.values = [int(v) for v in knot_values]
        self.boosts = [F64(b) for b in knot_boosts]
        self.unset = F64(unset_boost)
        assert 1 <= len(self.values) == len(self.boosts) <= MAX_KNOTS
        assert all(a < b for a, b in zip(self.values, self.values[1:])) and NO_VALUE not in self.values
        assert all(np.isfinite(b) for b in self.boosts) and np.isfinite(self.unset)

    @property
    def b_max(self):
        return max(self.boosts + [self.unset])

    def args(self):
        """what Searcher.search_boosted takes"""
        return self.values, [float(b) for b in self.boosts], float(self.unset)

    def __call__(self, v):
        """boost(v); v None or NO_VALUE: no value"""
        if v is None or v == NO_VALUE:
            return self.unset
        v = int(v)
        kv, kb = self.values, self.boosts
        if v <= kv[0]:
            return kb[0]
        if v >= kv[-1]:
            return kb[-1]
        j = max(i for i in range(len(kv) - 1) if kv[i] <= v)
        assert kv[j] <= v < kv[j + 1]
        num_int = (v - kv[j]) % (1 << 64)  # the wrapping 64-bit difference: exact for any pair of int64
        den_int = (kv[j + 1] - kv[j]) % (1 << 64)
        num = F64(float(num_int))  # (double)(uint64_t): one rounding, to nearest even
        den = F64(float(den_int))
        t = num / den
        d = kb[j + 1] - kb[j]
        p = t * d
        b = kb[j] + p
        lo = min(kb[j], kb[j + 1])
        hi = max(kb[j], kb[j + 1])
        if not b >= lo:
            b = lo
        if not b <= hi:
            b = hi
        return b


def relevance(c, metric, dim):
    c = F64(c)
    if metric == "dot":
        return c / F64(dim)
    return c


def order(m, ranks):
    """ranks sorted by (m descending, rank ascending)"""
    return sorted(ranks, key=lambda r: (-float(m[r]), r))


def walk_list(rel, values, boost, k, pool):
    """rel: the relevances of a ranked list, best first; values: their values (None / NO_VALUE: none).
    -> (kept ranks best first, m of the examined prefix [list], examined, exact)"""
    n = len(rel)
    b_max = boost.b_max
    m = []
    kept, examined = [], 0
    while True:
        ask = min(STEP, pool - examined)
        got = min(ask, n - examined)
        for r in range(examined, examined + got):
            b = boost(values[r])
            m.append(F64(rel[r]) + b)
        kept = order(m, kept + list(range(examined, examined + got)))[: min(k, examined + got)]
        examined += got
        if got < ask:  # (a) the list ended
            return kept, m, examined, True
        if len(kept) == k:  # (b) the certificate
            bound = F64(rel[examined - 1]) + b_max
            if m[kept[-1]] >= bound:
                return kept, m, examined, True
        if examined == pool:  # (c)
            return kept, m, examined, False


def brute_list(rel, values, boost, k):
    """the top k over ALL of the list by (m, rank) -> (ranks, m [list])"""
    m = [F64(rel[r]) + boost(values[r]) for r in range(len(rel))]
    return order(m, list(range(len(rel))))[:k], m


class Walk:
    """ranks (in L), ids, scores (reported f32), boosted (f64), values (int64), examined, exact"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class BoostReference:
    """The ranked list of every query (oracle.topk over all rows, to `depth`), the walk over it and the brute force."""

    def __init__(self, oracle, queries, rows, ids, metric, depth=None):
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.ids, self.metric, self.dim = np.asarray(ids, dtype=np.int64), metric, self.rows.shape[1]
        n = self.rows.shape[0]
        self.pos, self.sc, self.cnt = oracle.topk(queries, self.rows, min(depth or n, n), metric=1 if metric == "dot" else 0)

    def ranked(self, q, allowed=None):
        n = int(self.cnt[q])
        L, sc = self.pos[q, :n], self.sc[q, :n]
        if allowed is not None:
            ok = np.isin(L, allowed)
            L, sc = L[ok], sc[ok]
        return L, sc

    def _lists(self, q, table, allowed):
        L, sc = self.ranked(q, allowed)
        rel = [relevance(c, self.metric, self.dim) for c in sc.tolist()]
        values = [table.get(int(i)) for i in self.ids[L].tolist()]
        return L, sc, rel, values

    def _result(self, L, sc, values, ranks, m, examined, exact):
        rows = L[ranks] if ranks else np.zeros(0, np.int64)
        return Walk(ranks=np.array(ranks, dtype=np.int32), ids=self.ids[rows], scores=reported(sc[ranks] if ranks else [], self.metric, self.dim),
                    boosted=np.array([m[r] for r in ranks], dtype=np.float64),
                    values=np.array([NO_VALUE if values[r] is None else values[r] for r in ranks], dtype=np.int64), examined=examined, exact=bool(exact))

    def walk(self, q, k, pool, table, boost, allowed=None):
        """table: {item id: value}"""
        L, sc, rel, values = self._lists(q, table, allowed)
        kept, m, examined, exact = walk_list(rel, values, boost, k, pool)
        return self._result(L, sc, values, kept, m, examined, exact)

    def brute(self, q, k, table, boost, allowed=None):
        L, sc, rel, values = self._lists(q, table, allowed)
        ranks, m = brute_list(rel, values, boost, k)
        return self._result(L, sc, values, ranks, m, len(rel), True)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(got, want, q, k, rows_only=False):
    """got: what Searcher.search_boosted returned; want: a Walk of query q.  Everything is compared for equality, scores as f32 bits
    and boosted scores as f64 bits, and the fill values behind the kept rows.  rows_only: the kept rows alone (against the brute
    force, whose `examined` is the whole list)."""
    ids, scores, boosted, values, ranks, counts, examined, exact = got
    n = len(want.ranks)
    print("query %d: kept %d/%d examined %d/%d exact %s/%s" % (q, int(counts[q]), n, int(examined[q]), want.examined, bool(exact[q]), want.exact))
    assert ids.shape == (len(counts), k) and values.shape == ids.shape and ranks.shape == ids.shape and boosted.shape == ids.shape
    assert int(counts[q]) == n, (q, int(counts[q]), n)
    np.testing.assert_array_equal(ranks[q, :n], want.ranks)
    np.testing.assert_array_equal(ids[q, :n], want.ids)
    np.testing.assert_array_equal(values[q, :n], want.values)
    np.testing.assert_array_equal(bits32(scores[q, :n]), bits32(want.scores))
    np.testing.assert_array_equal(bits64(boosted[q, :n]), bits64(want.boosted))
    assert (ids[q, n:] == -1).all() and np.isnan(scores[q, n:]).all() and np.isnan(boosted[q, n:]).all()
    assert (values[q, n:] == NO_VALUE).all() and (ranks[q, n:] == -1).all()
    if not rows_only:
        assert int(examined[q]) == want.examined, (q, int(examined[q]), want.examined)
        assert bool(exact[q]) == want.exact, q
