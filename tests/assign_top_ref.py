"""What the top-m label tests share (test_assign_top_cpu.py, test_assign_top_gpu.py): the reference of pcv_searcher_assign_top and the
comparison with it.  A plain module, like assign_ref.py, whose method it extends to m labels.

assign_top_reference: the labels of row r are the j with c(r, j) = orc_canonical_score(labels[j], row_r, D, metric) defined and
c >= (double)min_score, ordered by (c descending, j ascending), the first m of them.  The oracle is called for every (row, label)
whose f64 score by numpy is at least (the row's m-th best numpy score - 1e-6) and at least (min_score - 1e-6), and for every entry
that is not a number there: the two f64 computations differ by some D * 2^-53 relative to |l||x|, so a label further below can be
neither among the oracle's m best nor within its bound, and every label that can be listed has the oracle's own score.  The tests
keep |l||x| of the rows they check under the dot metric small enough for that."""
import ctypes as C

import numpy as np

from assign_ref import bits, canonical_norms, reported  # noqa: F401  (the tests import them from here)

_FP = C.POINTER(C.c_float)


def _select(scored, m, min_score, metric, dim):
    """scored: [(c, j)] with c from the oracle -> the m best as (labels, reported scores)"""
    keep = [(c, j) for c, j in scored if c == c and c >= float(np.float32(min_score))]
    keep.sort(key=lambda t: (-t[0], t[1]))
    keep = keep[:m]
    return [j for _, j in keep], [reported(c, metric, dim) for c, _ in keep]


def _pack(n, K, m, per_row):
    out_l = np.full((n, m), -1, dtype=np.int32)
    out_s = np.full((n, m), np.nan, dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    for r, (labs, scores) in per_row.items():
        counts[r] = len(labs)
        out_l[r, : len(labs)] = labs
        out_s[r, : len(labs)] = scores
    label_rows = np.bincount(out_l[out_l >= 0], minlength=K).astype(np.int64)
    return out_l, out_s, counts, label_rows


def assign_top_reference(oracle, rows, labels, m, min_score=None, metric="cosine", part=None):
    """-> (labels [n, m] int32, scores [n, m] f32, counts [n] int32, label_rows [K] int64); part: bool [n], the rows that take part"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.float32)
    n, dim = rows.shape
    K = labels.shape[0]
    mode = 1 if metric == "dot" else 0
    bound = -np.inf if min_score is None else float(np.float32(min_score))
    part = np.ones(n, dtype=bool) if part is None else np.asarray(part, dtype=bool)
    R, L = rows.astype(np.float64), labels.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        G = R @ L.T
        if mode == 0:
            G = G / np.outer(np.sqrt(canonical_norms(rows)), np.sqrt(canonical_norms(labels)))
    lptr = [C.cast(labels.ctypes.data + j * dim * 4, _FP) for j in range(K)]
    per_row = {}
    for r in np.nonzero(part)[0]:
        g = G[r]
        ok = np.isfinite(g)
        near = ~ok
        fin = np.sort(g[ok])[::-1]
        if fin.size:
            mth = fin[m - 1] if fin.size >= m else -np.inf
            near = near | (ok & (g >= mth - 1e-6) & (g >= bound - 1e-6))
        xptr = C.cast(rows.ctypes.data + int(r) * dim * 4, _FP)
        scored = [(oracle.lib.orc_canonical_score(lptr[j], xptr, dim, mode), int(j)) for j in np.nonzero(near)[0]]
        per_row[int(r)] = _select(scored, m, bound, metric, dim)
    return _pack(n, K, m, per_row)


def brute_force(oracle, rows, labels, m, min_score=None, metric="cosine"):
    """the definition itself: every (label, row) through the oracle"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.float32)
    mode = 1 if metric == "dot" else 0
    bound = -np.inf if min_score is None else float(np.float32(min_score))
    per_row = {}
    for r in range(rows.shape[0]):
        scored = [(oracle.canonical_score(labels[j], rows[r], mode), j) for j in range(labels.shape[0])]
        per_row[r] = _select(scored, m, bound, metric, rows.shape[1])
    return _pack(rows.shape[0], labels.shape[0], m, per_row)


def check_assign_top(got, want, ids=None):
    labels, scores, got_ids, counts, label_rows = got
    w_labels, w_scores, w_counts, w_label_rows = want
    print("rows %d listed %d/%d" % (len(counts), int(counts.sum()), int(w_counts.sum())))
    np.testing.assert_array_equal(counts, w_counts)
    np.testing.assert_array_equal(labels, w_labels)
    np.testing.assert_array_equal(bits(scores), bits(w_scores))
    np.testing.assert_array_equal(label_rows, w_label_rows)
    if ids is not None:
        np.testing.assert_array_equal(got_ids, ids)
