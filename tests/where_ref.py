"""The reference of filtered search (pcv_searcher_search_where / _count_where), in Python: the ranked list L of a query comes from
oracle.topk over all rows, and the walk over it applies the predicate to a dict item id -> value.  A row's value is the value of its
item id; an id the dict does not hold (or holds as NO_VALUE) has none."""
import numpy as np

from grouped_ref import default_pool, reported  # noqa: F401  (the Python default of `pool` is grouped_ref's rule)

NO_VALUE = -(1 << 63)
UNSET_PASSES, OUTSIDE = 1, 2


def passes(v, lo, hi, flags):
    """the predicate: a value in [lo, hi] (OUTSIDE: a value not in it); no value: UNSET_PASSES alone decides"""
    if v is None or v == NO_VALUE:
        return bool(flags & UNSET_PASSES)
    return (lo <= v <= hi) != bool(flags & OUTSIDE)


def walk_list(L, scores, value_of_row, k, pool, lo, hi, flags):
    """L: the rows of a ranked list, best first; scores: their scores; value_of_row(row) -> value or NO_VALUE.
    -> (kept rows, their scores, their values, examined, more)"""
    kept, kept_sc, values, examined = [], [], [], 0
    for row, s in zip(list(L)[:pool], list(scores)[:pool]):
        examined += 1
        v = value_of_row(row)
        if not passes(v, lo, hi, flags):
            continue
        kept.append(row)
        kept_sc.append(s)
        values.append(NO_VALUE if v is None else int(v))
        if len(kept) == k:
            break
    more = len(kept) < k and examined == pool and len(L) > pool
    return kept, kept_sc, values, examined, more


def count(ids, table, lo, hi, flags):
    """how many of the rows carrying `ids` pass"""
    return sum(1 for i in np.asarray(ids).tolist() if passes(table.get(int(i)), lo, hi, flags))


class WhereReference:
    """The ranked list of every query (oracle.topk over all rows, to `depth`) and the walk over it."""

    def __init__(self, oracle, queries, rows, ids, metric, depth=None):
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.ids, self.metric, self.dim = np.asarray(ids, dtype=np.int64), metric, self.rows.shape[1]
        n = self.rows.shape[0]
        self.pos, self.sc, self.cnt = oracle.topk(queries, self.rows, min(depth or n, n), metric=1 if metric == "dot" else 0)

    def ranked(self, q, allowed=None):
        """rows and f64 scores of query q's list, restricted to the rows in `allowed` (hidden rows, a view, a source filter)"""
        n = int(self.cnt[q])
        L, sc = self.pos[q, :n], self.sc[q, :n]
        if allowed is not None:
            ok = np.isin(L, allowed)
            L, sc = L[ok], sc[ok]
        return L, sc

    def walk(self, q, k, pool, table, lo, hi, flags=0, allowed=None):
        """table: {item id: value}.  -> (ids, f32 scores, values, examined, more)"""
        L, sc = self.ranked(q, allowed)
        kept, kept_sc, values, examined, more = walk_list(
            L.tolist(), sc.tolist(), lambda row: table.get(int(self.ids[row])), k, pool, lo, hi, flags)
        ids = self.ids[kept] if kept else np.zeros(0, np.int64)
        return ids, reported(kept_sc, self.metric, self.dim), np.array(values, dtype=np.int64), examined, more


def check(got, want, q, k):
    """got: what Searcher.search_where returned; want: WhereReference.walk of query q.  Everything is compared exactly, scores by bits."""
    ids, scores, values, counts, examined, more = got
    w_ids, w_scores, w_values, w_examined, w_more = want
    n = len(w_ids)
    print("query %d: kept %d/%d examined %d/%d more %s/%s" % (q, int(counts[q]), n, int(examined[q]), w_examined, bool(more[q]), w_more))
    assert ids.shape == (len(counts), k) and values.shape == ids.shape
    assert int(counts[q]) == n, (q, int(counts[q]), n)
    np.testing.assert_array_equal(ids[q, :n], w_ids)
    np.testing.assert_array_equal(np.ascontiguousarray(scores[q, :n]).view(np.uint32), np.ascontiguousarray(w_scores, dtype=np.float32).view(np.uint32))
    np.testing.assert_array_equal(values[q, :n], w_values)
    assert int(examined[q]) == w_examined, (q, int(examined[q]), w_examined)
    assert bool(more[q]) == w_more, q
    assert (ids[q, n:] == -1).all() and np.isnan(scores[q, n:]).all() and (values[q, n:] == NO_VALUE).all()
