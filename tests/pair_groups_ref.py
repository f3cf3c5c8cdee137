"""What the group-aware pair tests share (test_pair_groups_cpu.py, test_pair_groups_gpu.py): the reference of
pcv_searcher_neighbors_grouped, pcv_searcher_match_grouped and pcv_searcher_find_duplicates_grouped, and the comparison with it.  A
plain module, like neighbors_ref.py and match_ref.py, which it extends with a group per ROW and the two flags.

`groups` is one int64 per stored row: the value the row's item id has in the group table, -1 for none.  Two different rows are siblings
iff both have a group >= 0 and the keys are equal.

SKIP_OWN masks the owner's siblings to -inf before the k-th numpy cosine is taken.  ONE_PER_GROUP first runs the collapse walk on the
numpy cosines to get the k-th kept cosine v, then sends every partner with numpy cosine >= v - 1e-6 through the oracle, sorts by
(-c, position) and walks: the numpy walk shows k different groups whose best member has numpy cosine >= v, the two f64 computations
differ by D * 2^-53 at most, so the oracle's k-th kept cosine is above v - 1e-6 and every partner the oracle's walk visits up to its
k-th kept one is among those sent."""
import ctypes as C

import numpy as np

from duplicates_ref import bits
from neighbors_ref import canonical_norm2, takes_part

SKIP_OWN, ONE_PER_GROUP = 1, 2
NO_GROUP = -1
_FP = C.POINTER(C.c_float)


def row_groups(ids, table):
    """the group of every row: `table` maps item id -> group (an id that is missing, or mapped to -1: none)"""
    return np.array([table.get(int(i), NO_GROUP) for i in ids], dtype=np.int64)


def _bound(min_score):
    lo = np.float32(min_score)
    return None if lo == np.float32(-1.0) else float(lo)


def _walk(found, groups, k, flags, lo_c):
    """found: (-c, position) ascending.  -> the kept ones: the first k, or under ONE_PER_GROUP the first k whose group no kept one has"""
    kept, seen = [], set()
    for c, p in found:
        if lo_c is not None and -c < lo_c:
            break
        g = int(groups[p])
        if (flags & ONE_PER_GROUP) and g >= 0:
            if g in seen:
                continue
            seen.add(g)
        kept.append((c, p))
        if len(kept) == k:
            break
    return kept


def _empty(n, k):
    return (np.full((n, k), -1, dtype=np.int64), np.full((n, k), np.nan, dtype=np.float32), np.full((n, k), NO_GROUP, dtype=np.int64),
            np.zeros(n, dtype=np.int32))


def _store(out, o, kept, ids, groups):
    nbr, score, grp, counts = out
    counts[o] = len(kept)
    for j, (c, p) in enumerate(kept):
        nbr[o, j] = ids[p]
        score[o, j] = np.float32(-c)
        grp[o, j] = groups[p]


def _setup(rows, ids, groups, owner, partner, part):
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    total = rows.shape[0]
    ids = np.asarray(ids, dtype=np.int64)
    groups = np.asarray(groups, dtype=np.int64)
    assert groups.shape == (total,)
    owner = np.ones(total, dtype=bool) if owner is None else np.asarray(owner, dtype=bool)
    partner = np.ones(total, dtype=bool) if partner is None else np.asarray(partner, dtype=bool)
    live = takes_part(rows, part)
    return rows, ids, groups, owner, np.nonzero(owner & live)[0], np.nonzero(partner & live)[0]


def reference(oracle, rows, ids, groups, k, flags, owner=None, partner=None, min_score=-1.0, part=None):
    """-> (ids [n], partner ids [n, k] (-1), f32 scores [n, k] (NaN), partner groups [n, k] (-1), counts [n] int32) of the n owner rows
    by position.  owner / partner None: every row (the neighbours); `part`: the rows a search could return (None: all)"""
    rows, ids, groups, owner, own, par = _setup(rows, ids, groups, owner, partner, part)
    dim = rows.shape[1]
    out_of = np.cumsum(owner) - 1
    n = int(owner.sum())
    out = _empty(n, k)
    lo_c = _bound(min_score)
    if par.size and own.size:
        V = rows[par].astype(np.float64) / np.sqrt(canonical_norm2(rows[par]))[:, None]
        gpar = groups[par]
        ptr = {int(r): C.cast(rows.ctypes.data + int(r) * dim * 4, _FP) for r in np.union1d(own, par)}
        for lo in range(0, own.size, 1024):
            chunk = own[lo : lo + 1024]
            G = (rows[chunk].astype(np.float64) / np.sqrt(canonical_norm2(rows[chunk]))[:, None]) @ V.T
            for i, r in enumerate(chunk):
                r = int(r)
                g = G[i]
                g[par == r] = -np.inf  # a row is no partner of itself
                if (flags & SKIP_OWN) and groups[r] >= 0:
                    g[gpar == groups[r]] = -np.inf
                avail = np.nonzero(g > -np.inf)[0]
                if avail.size == 0:
                    continue
                if flags & ONE_PER_GROUP:
                    order = avail[np.lexsort((par[avail], -g[avail]))]
                    kept = _walk([(-g[j], int(par[j])) for j in order], groups, k, flags, None)
                    v = -kept[-1][0] if len(kept) == k else -np.inf
                else:
                    kk = min(k, avail.size)
                    v = np.partition(g, g.size - kk)[g.size - kk]
                near = par[avail[g[avail] >= v - 1e-6]]
                found = sorted((-oracle.lib.orc_canonical_score(ptr[r], ptr[int(p)], dim, 0), int(p)) for p in near)
                _store(out, out_of[r], _walk(found, groups, k, flags, lo_c), ids, groups)
    return (ids[owner].copy(),) + out


def brute_force(oracle, rows, ids, groups, k, flags, owner=None, partner=None, min_score=-1.0, part=None):
    """the definition itself, every pair through the oracle: for small inputs, to check `reference`"""
    rows, ids, groups, owner, own, par = _setup(rows, ids, groups, owner, partner, part)
    out_of = np.cumsum(owner) - 1
    n = int(owner.sum())
    out = _empty(n, k)
    lo_c = _bound(min_score)
    for r in own:
        scored = []
        for p in par:
            if p == r or ((flags & SKIP_OWN) and groups[r] >= 0 and groups[r] == groups[p]):
                continue
            scored.append((-oracle.canonical_score(rows[r], rows[p]), int(p)))
        _store(out, out_of[r], _walk(sorted(scored), groups, k, flags, lo_c), ids, groups)
    return (ids[owner].copy(),) + out


def check(got, want):
    """neighbors_ref.check with the partners' groups beside the ids: ids, counts, the f32 bits of the scores, groups"""
    g_ids, g_nbr, g_score, g_grp, g_counts = got
    w_ids, w_nbr, w_score, w_grp, w_counts = want
    print("rows %d/%d listed %d/%d" % (len(g_ids), len(w_ids), int(g_counts.sum()), int(w_counts.sum())))
    assert g_nbr.shape == w_nbr.shape and g_score.shape == w_score.shape and g_grp.shape == w_grp.shape and g_counts.dtype == np.int32
    np.testing.assert_array_equal(g_ids, w_ids)
    np.testing.assert_array_equal(g_counts, w_counts)
    np.testing.assert_array_equal(g_nbr, w_nbr)
    np.testing.assert_array_equal(g_grp, w_grp)
    used = np.arange(w_nbr.shape[1])[None, :] < w_counts[:, None]
    np.testing.assert_array_equal(bits(g_score)[used], bits(w_score)[used])
    assert np.isnan(g_score[~used]).all()


def duplicates(oracle, rows, ids, groups, threshold, part=None):
    """-> (id_a, id_b, f32 scores, skipped): duplicates_ref.reference without the sibling pairs, which `skipped` counts.  `part`: positions"""
    import duplicates_ref

    rows = np.ascontiguousarray(rows, dtype=np.float32)
    part = np.arange(rows.shape[0]) if part is None else np.asarray(part, dtype=np.int64)
    # the plain reference over positions instead of ids, so that a pair's rows — and their groups — are known
    pa_, pb_, sc = duplicates_ref.reference(oracle, rows, np.arange(rows.shape[0], dtype=np.int64), threshold, part)
    groups = np.asarray(groups, dtype=np.int64)
    sib = (groups[pa_] >= 0) & (groups[pa_] == groups[pb_])
    ids = np.asarray(ids, dtype=np.int64)
    return ids[pa_[~sib]], ids[pb_[~sib]], sc[~sib], int(sib.sum())
