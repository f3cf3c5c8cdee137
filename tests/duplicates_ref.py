"""What the duplicate-pair tests share (test_duplicates_gpu.py, test_duplicates_paths_gpu.py): the reference of
pcv_searcher_find_duplicates, the comparison with it, and the helpers that build a corpus.  A plain module, like oracle_ffi.py.

The reference of every check is orc_canonical_score(row_a, row_b, D, 0) >= (double)threshold over all a < b of the participating
rows, sorted (-c, a, b).  It calls the oracle for every pair whose f64 cosine by numpy is within 1e-6 of the threshold or above it:
the two f64 computations differ by D * 2^-53 at most, so a pair further below cannot reach the threshold in the oracle either."""
import ctypes as C

import numpy as np

import perceive_amd as pa

_FP = C.POINTER(C.c_float)
_CHUNK = 1024  # rows of one side of a Gram block: 8 MB of f64 per block, whatever the corpus


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def reference(oracle, rows, ids, threshold, part=None):
    """-> (id_a, id_b, f32 scores) of all duplicate pairs among rows[part] (positions ascending; None: all rows), in the call's order"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    part = np.arange(rows.shape[0]) if part is None else np.asarray(part, dtype=np.int64)
    thr = float(np.float32(threshold))  # (double)threshold
    R = rows[part].astype(np.float64)
    nrm = np.sqrt((R * R).sum(axis=1))
    n = R.shape[0]
    ia, ib = [], []
    for lo_a in range(0, n, _CHUNK):
        hi_a = min(n, lo_a + _CHUNK)
        for lo_b in range(lo_a, n, _CHUNK):
            hi_b = min(n, lo_b + _CHUNK)
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                G = (R[lo_a:hi_a] @ R[lo_b:hi_b].T) / np.outer(nrm[lo_a:hi_a], nrm[lo_b:hi_b])
            near = G >= thr - 1e-6
            if lo_a == lo_b:
                near = np.triu(near, k=1)
            a, b = np.nonzero(near)
            ia.append(a + lo_a)
            ib.append(b + lo_b)
    ia = np.concatenate(ia) if ia else np.zeros(0, dtype=np.int64)
    ib = np.concatenate(ib) if ib else np.zeros(0, dtype=np.int64)
    dim = rows.shape[1]
    ptr = {int(i): C.cast(rows.ctypes.data + int(part[i]) * dim * 4, _FP) for i in np.union1d(ia, ib)}
    found = []
    for a, b in zip(ia.tolist(), ib.tolist()):
        c = oracle.lib.orc_canonical_score(ptr[a], ptr[b], dim, 0)
        if c >= thr:
            found.append((-c, a, b))
    found.sort()
    a = np.array([part[f[1]] for f in found], dtype=np.int64)
    b = np.array([part[f[2]] for f in found], dtype=np.int64)
    c = np.array([-f[0] for f in found], dtype=np.float64)
    return ids[a], ids[b], c.astype(np.float32)


def check(got, want, max_pairs=None):
    id_a, id_b, scores, total = got
    w_a, w_b, w_s = want
    n = len(w_a) if max_pairs is None else min(len(w_a), max_pairs)
    print("pairs %d/%d total %d/%d" % (len(id_a), n, total, len(w_a)))
    assert total == len(w_a)
    assert len(id_a) == len(id_b) == len(scores) == n
    np.testing.assert_array_equal(id_a, w_a[:n])
    np.testing.assert_array_equal(id_b, w_b[:n])
    np.testing.assert_array_equal(bits(scores), bits(w_s[:n]))


def neighbour(rng, a, cos):
    """a row at cosine `cos` of a (up to the f32 rounding of its features), of a's norm"""
    a64 = a.astype(np.float64)
    u = rng.standard_normal(a.shape[0])
    u -= (u @ a64) / (a64 @ a64) * a64
    u *= np.linalg.norm(a64) / np.linalg.norm(u)
    return (cos * a64 + np.sqrt(max(0.0, 1.0 - cos * cos)) * u).astype(np.float32)


def make_ids(rng, n):
    return (rng.permutation(n) * 7 + 1000).astype(np.int64)


def build(ctx, rows, ids, metric="cosine", sources=None):
    """sources: [(source id, first row, end row)]; None: everything in source 1"""
    s = pa.Searcher(ctx, rows.shape[1], metric)
    for sid, lo, hi in sources or [(1, 0, rows.shape[0])]:
        s.add_rows(sid, rows[lo:hi], ids[lo:hi])
    s.finalize()
    return s


def bf16_rne(x):
    """f32 -> bf16, round to nearest even, by integer arithmetic on the bits; returned as the f32 of the same value (finite input)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def screen_score(a, b):
    """The screen's score in exact arithmetic: the f64 dot product of the two rows rounded to bf16 over the canonical norms (f64,
    feature order) of the unrounded rows.  It shows how hostile a test's input is to the bf16 screen; it is never an expected result."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    dot = float(np.cumsum(bf16_rne(a).astype(np.float64) * bf16_rne(b).astype(np.float64))[-1])
    na = float(np.cumsum(a.astype(np.float64) ** 2)[-1])
    nb = float(np.cumsum(b.astype(np.float64) ** 2)[-1])
    return dot / (np.sqrt(na) * np.sqrt(nb))
