"""What the item-match tests share (test_match_cpu.py, test_match_gpu.py): the reference of pcv_searcher_match and the comparison
with it.  A plain module, like neighbors_ref.py, which it generalises with an owner mask, a partner mask and a score bound.

`rows` and `ids` are the stored rows in global position order; `owner` marks the rows of the `from` sources (the rows concerned, which
the outputs list in that order), `partner` the rows of the `to` sources, `part` the rows a search could return (None: all).  The
reference of every check is orc_canonical_score(row_r, row_p, D, 0) for every participating owner r and every participating partner p
at another position: the k largest by (-c, position) among those with c >= float64(float32(min_score)) (min_score == -1: all).  It
builds the f64 Gram of the owners against the partners in chunks and calls the oracle for every partner whose f64 cosine by numpy is
within 1e-6 of the row's kk-th numpy cosine, or above it, kk = min(k, partners - [the owner is one]): the two f64 computations differ
by D * 2^-53 at most, so a partner further below cannot be among the oracle's kk best either; the bound then drops what is below it."""
import ctypes as C

import numpy as np

from neighbors_ref import canonical_norm2, check, takes_part  # noqa: F401  (check: the comparison is the neighbours')

_FP = C.POINTER(C.c_float)
_CHUNK = 1024  # owners of one Gram block


def _bound(min_score):
    """(double)min_score, or None where the call skips the comparison"""
    lo = np.float32(min_score)
    return None if lo == np.float32(-1.0) else float(lo)


def _masks(n, owner, partner, rows, part):
    owner = np.ones(n, dtype=bool) if owner is None else np.asarray(owner, dtype=bool)
    partner = np.ones(n, dtype=bool) if partner is None else np.asarray(partner, dtype=bool)
    live = takes_part(rows, part)
    return owner, np.nonzero(owner & live)[0], np.nonzero(partner & live)[0]


def reference(oracle, rows, ids, owner, partner, k, min_score=-1.0, part=None):
    """-> (ids [n], match_ids [n, k] (-1), f32 scores [n, k] (NaN), counts [n] int32) of the n owner rows by position, as the call
    orders them"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    total, dim = rows.shape
    ids = np.asarray(ids, dtype=np.int64)
    owner, own, par = _masks(total, owner, partner, rows, part)
    out_of = np.cumsum(owner) - 1  # position -> output index
    n = int(owner.sum())
    mids = np.full((n, k), -1, dtype=np.int64)
    score = np.full((n, k), np.nan, dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    lo_c = _bound(min_score)
    P = par.size
    if P >= 1 and own.size >= 1:
        V = rows[par].astype(np.float64) / np.sqrt(canonical_norm2(rows[par]))[:, None]
        ptr = {int(r): C.cast(rows.ctypes.data + int(r) * dim * 4, _FP) for r in np.union1d(own, par)}
        slot_of = {int(p): j for j, p in enumerate(par)}
        for lo in range(0, own.size, _CHUNK):
            chunk = own[lo : lo + _CHUNK]
            U = rows[chunk].astype(np.float64) / np.sqrt(canonical_norm2(rows[chunk]))[:, None]
            G = U @ V.T
            for i, r in enumerate(chunk):
                r = int(r)
                g = G[i]
                if r in slot_of:
                    g[slot_of[r]] = -np.inf  # a row is no partner of itself
                kk = min(k, P - (1 if r in slot_of else 0))
                if kk == 0:
                    continue
                kth = np.partition(g, P - kk)[P - kk]
                near = par[np.nonzero(g >= kth - 1e-6)[0]]
                found = sorted((-oracle.lib.orc_canonical_score(ptr[r], ptr[int(p)], dim, 0), int(p)) for p in near)[:kk]
                if lo_c is not None:
                    found = [(c, p) for c, p in found if -c >= lo_c]
                o = out_of[r]
                counts[o] = len(found)
                mids[o, : len(found)] = ids[[p for _c, p in found]]
                score[o, : len(found)] = np.array([-c for c, _p in found], dtype=np.float64).astype(np.float32)
    return ids[owner].copy(), mids, score, counts


def brute_force(oracle, rows, ids, owner, partner, k, min_score=-1.0, part=None):
    """the definition itself, every pair through the oracle: for small inputs, to check `reference`"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    total = rows.shape[0]
    ids = np.asarray(ids, dtype=np.int64)
    owner, own, par = _masks(total, owner, partner, rows, part)
    out_of = np.cumsum(owner) - 1
    n = int(owner.sum())
    mids = np.full((n, k), -1, dtype=np.int64)
    score = np.full((n, k), np.nan, dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    lo_c = _bound(min_score)
    for r in own:
        scored = [(-oracle.canonical_score(rows[r], rows[p]), int(p)) for p in par if p != r]
        found = sorted((c, p) for c, p in scored if lo_c is None or -c >= lo_c)[:k]
        o = out_of[r]
        counts[o] = len(found)
        for j, (c, p) in enumerate(found):
            mids[o, j] = ids[p]
            score[o, j] = np.float32(-c)
    return ids[owner].copy(), mids, score, counts
