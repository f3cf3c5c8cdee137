"""The reference of grouped results (pcv_searcher_search_grouped), in Python: the ranked list L of a query comes from oracle.topk
over all rows, and the walk over it is a dict of kept group -> output slot.  A row's group is the group of its item id; a row whose
id has none (no entry, or PCV_NO_GROUP) is a group of its own — the row, not the id."""
import numpy as np

NO_GROUP = -1


def reported(c, metric, dim):
    """hits_to_outputs: (float)c for cosine, max(0, 1 - c / dim) in f64 then f32 for the dot metric"""
    c = np.asarray(c, dtype=np.float64)
    if metric == "dot":
        d = 1.0 - c / np.float64(dim)
        return np.where(d > 0.0, d, 0.0).astype(np.float32)
    return c.astype(np.float32)


def default_pool(k):
    return min(4096, max(128, 8 * k))


def walk_list(L, scores, group_of_row, k, pool):
    """L: the rows of a ranked list, best first; scores: their scores; group_of_row(row) -> key >= 0 or NO_GROUP.
    -> (kept rows, their scores, their groups, collapsed per kept row, examined, more)"""
    slot_of = {}
    kept, kept_sc, groups, collapsed, examined = [], [], [], [], 0
    for row, s in zip(list(L)[:pool], list(scores)[:pool]):
        examined += 1
        g = int(group_of_row(row))
        if g >= 0 and g in slot_of:
            collapsed[slot_of[g]] += 1
            continue
        if g >= 0:
            slot_of[g] = len(kept)
        kept.append(row)
        kept_sc.append(s)
        groups.append(g if g >= 0 else NO_GROUP)
        collapsed.append(0)
        if len(kept) == k:
            break
    more = len(kept) < k and examined == pool and len(L) > pool
    return kept, kept_sc, groups, collapsed, examined, more


class GroupedReference:
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

    def walk(self, q, k, pool, groups, allowed=None):
        """groups: {item id: group key}.  -> (ids, f32 scores, groups, collapsed, examined, more)"""
        L, sc = self.ranked(q, allowed)
        kept, kept_sc, kg, collapsed, examined, more = walk_list(
            L.tolist(), sc.tolist(), lambda row: groups.get(int(self.ids[row]), NO_GROUP), k, pool)
        ids = self.ids[kept] if kept else np.zeros(0, np.int64)
        return ids, reported(kept_sc, self.metric, self.dim), np.array(kg, dtype=np.int64), np.array(collapsed, dtype=np.int32), examined, more


def check(got, want, q, k):
    """got: what Searcher.search_grouped returned; want: GroupedReference.walk of query q.  Everything is compared exactly, scores by bits."""
    ids, scores, groups, counts, collapsed, examined, more = got
    w_ids, w_scores, w_groups, w_collapsed, w_examined, w_more = want
    n = len(w_ids)
    print("query %d: kept %d/%d examined %d/%d more %s/%s" % (q, int(counts[q]), n, int(examined[q]), w_examined, bool(more[q]), w_more))
    assert ids.shape == (len(counts), k) and groups.shape == ids.shape and collapsed.shape == ids.shape
    assert int(counts[q]) == n, (q, int(counts[q]), n)
    np.testing.assert_array_equal(ids[q, :n], w_ids)
    np.testing.assert_array_equal(np.ascontiguousarray(scores[q, :n]).view(np.uint32), np.ascontiguousarray(w_scores, dtype=np.float32).view(np.uint32))
    np.testing.assert_array_equal(groups[q, :n], w_groups)
    np.testing.assert_array_equal(collapsed[q, :n], w_collapsed)
    assert int(examined[q]) == w_examined, (q, int(examined[q]), w_examined)
    assert bool(more[q]) == w_more, q
    assert (ids[q, n:] == -1).all() and np.isnan(scores[q, n:]).all() and (groups[q, n:] == NO_GROUP).all() and (collapsed[q, n:] == 0).all()
