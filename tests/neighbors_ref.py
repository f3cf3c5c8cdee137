"""What the item-neighbour tests share (test_neighbors_cpu.py, test_neighbors_gpu.py): the reference of pcv_searcher_neighbors and
the comparison with it.  A plain module, like duplicates_ref.py, whose corpus helpers the tests use beside it.

The reference of every check is orc_canonical_score(row_r, row_p, D, 0) for every participating r and every other participating p,
the k largest by (-c, position).  It builds the f64 Gram in chunks and calls the oracle for every partner whose f64 cosine by numpy
is within 1e-6 of the row's k-th numpy cosine, or above it: the two f64 computations differ by D * 2^-53 at most, so a partner
further below cannot be among the oracle's k best either."""
import ctypes as C

import numpy as np

from duplicates_ref import bits

_FP = C.POINTER(C.c_float)
_CHUNK = 1024  # owners of one Gram block


def canonical_norm2(rows):
    """|x|^2 in f64, products exact, summed in feature order"""
    r = np.ascontiguousarray(rows, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        return np.cumsum(r * r, axis=1)[:, -1]


def takes_part(rows, part=None):
    """the rows with a cosine (canonical |x|^2 in [2^-126, inf)) among those a search could return (`part`: bool per row; None: all)"""
    n2 = canonical_norm2(rows)
    ok = (n2 >= 2.0 ** -126) & (n2 < np.inf)
    return ok if part is None else ok & np.asarray(part, dtype=bool)


def reference(oracle, rows, ids, k, part=None):
    """-> (ids [n], neighbor_ids [n, k] (-1), f32 scores [n, k] (NaN), counts [n] int32) by position, as the call orders them"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dim = rows.shape
    ids = np.asarray(ids, dtype=np.int64)
    live = np.nonzero(takes_part(rows, part))[0]
    nbr = np.full((n, k), -1, dtype=np.int64)
    score = np.full((n, k), np.nan, dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    P = live.size
    if P >= 2:
        R = rows[live].astype(np.float64)
        nrm = np.sqrt(canonical_norm2(rows[live]))
        U = R / nrm[:, None]  # (wild rows: the division is exact enough for a 1e-6 window, the decision is the oracle's)
        ptr = [C.cast(rows.ctypes.data + int(r) * dim * 4, _FP) for r in live]
        kk = min(k, P - 1)
        for lo in range(0, P, _CHUNK):
            hi = min(P, lo + _CHUNK)
            G = U[lo:hi] @ U.T
            G[np.arange(hi - lo), np.arange(lo, hi)] = -np.inf  # a row is no partner of itself
            kth = np.partition(G, P - kk, axis=1)[:, P - kk]
            for i in range(lo, hi):
                near = np.nonzero(G[i - lo] >= kth[i - lo] - 1e-6)[0]
                found = sorted((-oracle.lib.orc_canonical_score(ptr[i], ptr[int(j)], dim, 0), int(j)) for j in near)[:kk]
                r = live[i]
                counts[r] = kk
                nbr[r, :kk] = ids[live[[j for _c, j in found]]]
                score[r, :kk] = np.array([-c for c, _j in found], dtype=np.float64).astype(np.float32)
    return ids.copy(), nbr, score, counts


def check(got, want):
    g_ids, g_nbr, g_score, g_counts = got
    w_ids, w_nbr, w_score, w_counts = want
    print("rows %d/%d listed %d/%d" % (len(g_ids), len(w_ids), int(g_counts.sum()), int(w_counts.sum())))
    assert g_nbr.shape == w_nbr.shape and g_score.shape == w_score.shape and g_counts.dtype == np.int32
    np.testing.assert_array_equal(g_ids, w_ids)
    np.testing.assert_array_equal(g_counts, w_counts)
    np.testing.assert_array_equal(g_nbr, w_nbr)
    used = np.arange(w_nbr.shape[1])[None, :] < w_counts[:, None]
    np.testing.assert_array_equal(bits(g_score)[used], bits(w_score)[used])
    assert np.isnan(g_score[~used]).all()


def brute_force(oracle, rows, ids, k, part=None):
    """the definition itself, every pair through the oracle: for small inputs, to check `reference`"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dim = rows.shape
    live = np.nonzero(takes_part(rows, part))[0]
    nbr = np.full((n, k), -1, dtype=np.int64)
    score = np.full((n, k), np.nan, dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    for r in live:
        found = sorted((-oracle.canonical_score(rows[r], rows[p]), int(p)) for p in live if p != r)[:k]
        counts[r] = len(found)
        for j, (c, p) in enumerate(found):
            nbr[r, j] = ids[p]
            score[r, j] = np.float32(-c)
    return np.asarray(ids, dtype=np.int64).copy(), nbr, score, counts
