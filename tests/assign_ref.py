"""What the item-label tests share (test_assign_cpu.py, test_assign_gpu.py): the references of pcv_searcher_assign, _label_sums and
_kmeans and the comparison with them.  A plain module, like duplicates_ref.py.

assign_reference: label(r) = the j with the largest defined orc_canonical_score(labels[j], row_r, D, metric), ties to the lower j.
It calls the oracle for every (label, row) whose f64 score by numpy is within 1e-6 of the row's best (or is not a number there): the
two f64 computations differ by some D * 2^-53 relative to |l||x|, so a label further below cannot be the oracle's best either.  The
tests keep |l||x| of the rows they check under the dot metric small enough for that."""
import ctypes as C

import numpy as np

from duplicates_ref import bits  # noqa: F401  (the tests import it from here)

_FP = C.POINTER(C.c_float)


def canonical_norms(rows):
    """the canonical |x|^2: f64, feature order"""
    r = np.ascontiguousarray(rows, dtype=np.float32).astype(np.float64)
    return np.cumsum(r * r, axis=1)[:, -1]


def reported(c, metric, dim):
    """the f32 score a search reports for the canonical score c"""
    if metric == "dot":
        d = 1.0 - c / float(dim)
        return np.float32(d if d > 0.0 else 0.0)
    return np.float32(c)


def assign_reference(oracle, rows, labels, metric="cosine", part=None):
    """-> (label [n] int32, score [n] f32, counts [K] int64); part: bool [n], the rows that take part (None: all)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.float32)
    n, dim = rows.shape
    K = labels.shape[0]
    m = 1 if metric == "dot" else 0
    part = np.ones(n, dtype=bool) if part is None else np.asarray(part, dtype=bool)
    R, L = rows.astype(np.float64), labels.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        G = R @ L.T
        if m == 0:
            G = G / np.outer(np.sqrt(canonical_norms(rows)), np.sqrt(canonical_norms(labels)))
    lptr = [C.cast(labels.ctypes.data + j * dim * 4, _FP) for j in range(K)]
    out_l = np.full(n, -1, dtype=np.int32)
    out_s = np.full(n, np.nan, dtype=np.float32)
    for r in np.nonzero(part)[0]:
        g = G[r]
        ok = np.isfinite(g)
        near = ~ok
        if ok.any():
            near = near | (g >= g[ok].max() - 1e-6)
        xptr = C.cast(rows.ctypes.data + int(r) * dim * 4, _FP)
        best, bj = None, -1
        for j in np.nonzero(near)[0]:
            c = oracle.lib.orc_canonical_score(lptr[j], xptr, dim, m)
            if c == c and (best is None or c > best):
                best, bj = c, int(j)
        if bj >= 0:
            out_l[r] = bj
            out_s[r] = reported(best, metric, dim)
    return out_l, out_s, np.bincount(out_l[out_l >= 0], minlength=K).astype(np.int64)


def brute_force(oracle, rows, labels, metric="cosine"):
    """the definition itself: every (label, row) through the oracle"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.float32)
    m = 1 if metric == "dot" else 0
    out_l = np.full(rows.shape[0], -1, dtype=np.int32)
    out_s = np.full(rows.shape[0], np.nan, dtype=np.float32)
    for r in range(rows.shape[0]):
        best = None
        for j in range(labels.shape[0]):
            c = oracle.canonical_score(labels[j], rows[r], m)
            if c == c and (best is None or c > best):
                best, out_l[r] = c, j
        if best is not None:
            out_s[r] = reported(best, metric, rows.shape[1])
    return out_l, out_s


def unit_ints(rows):
    """t(r, d) = rint(x * rinv * 2^32) as int64 (one rounding, half to even) and which rows have a cosine"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n2 = canonical_norms(rows)
    has = (n2 >= 2.0 ** -126) & np.isfinite(n2)
    rinv = np.zeros(rows.shape[0], dtype=np.float32)
    rinv[has] = (1.0 / np.sqrt(n2[has])).astype(np.float32)
    t = np.rint(rows.astype(np.float64) * rinv.astype(np.float64)[:, None] * 2.0 ** 32).astype(np.int64)
    return t, has


def sums_reference(rows, lab, K, part=None):
    """-> (S [K, dim] int64, members [K] int64); part: bool [n], the rows that take part (None: all) — the others add nothing"""
    t, has = unit_ints(rows)
    if part is not None:
        has = has & np.asarray(part, dtype=bool)
    S = np.zeros((K, rows.shape[1]), dtype=np.int64)
    members = np.zeros(K, dtype=np.int64)
    for j in range(K):
        sel = (np.asarray(lab) == j) & has
        S[j] = t[sel].sum(axis=0)
        members[j] = sel.sum()
    return S, members


def kmeans_reference(oracle, rows, init, max_iters, part=None):
    """-> (centroids, label, score, counts, iterations, moved)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    cent = np.array(init, dtype=np.float32)
    K = cent.shape[0]
    prev = np.full(rows.shape[0], -1, dtype=np.int32)
    moved, updates = [], 0
    while True:
        lab, score, counts = assign_reference(oracle, rows, cent, "cosine", part)
        moved.append(int((lab != prev).sum()))
        if moved[-1] == 0 or updates == max_iters:
            break
        S, members = sums_reference(rows, lab, K)
        for j in range(K):
            if members[j]:
                cent[j] = (S[j].astype(np.float64) * 2.0 ** -32).astype(np.float32)
        updates += 1
        prev = lab
    return cent, lab, score, counts, updates, np.array(moved, dtype=np.int64)


def check_assign(got, want, ids=None):
    label, score, got_ids, counts = got
    w_label, w_score, w_counts = want
    print("rows %d labelled %d/%d" % (len(label), (label >= 0).sum(), (w_label >= 0).sum()))
    np.testing.assert_array_equal(label, w_label)
    np.testing.assert_array_equal(bits(score), bits(w_score))
    np.testing.assert_array_equal(counts, w_counts)
    if ids is not None:
        np.testing.assert_array_equal(got_ids, ids)
