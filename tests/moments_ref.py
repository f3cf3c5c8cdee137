"""What the moment tests share (test_moments_cpu.py, test_moments_gpu.py): the references of pcv_searcher_moments, _principal_axes
and _project and the comparison with them.  A plain module, like seeds_ref.py.

Moments: t(r, d) is assign_ref.unit_ints, the rows that take part are neighbors_ref.takes_part; S and C = T^T T are computed in
Python ints (object arrays), and the matrix is float(int) * 2.0**-64 — CPython rounds an int to the nearest float, ties to even.
`limb_matrices` is the same C from the three int64 limb products, exact in int64 for up to 2^30 rows: the form the device computes
and the reference of the large case.  Projection: np.add.accumulate over the f64 products starting from +0 (strictly sequential,
what pair_sums does), then * rinv, - offset, astype(float32), every step rounded on its own."""
import numpy as np

from assign_ref import canonical_norms, unit_ints
from duplicates_ref import bits
from neighbors_ref import takes_part

SCALE = 2.0 ** -64


def participating_ints(rows, part=None):
    """-> (t [n_part, dim] int64 of the participating rows, their indices)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    t, has = unit_ints(rows)
    live = takes_part(rows, part)
    assert not (live & ~has).any()
    idx = np.nonzero(live)[0]
    return t[idx], idx


def exact_moments(t):
    """-> (S [dim] object, C [dim, dim] object): Python ints"""
    T = t.astype(object)
    dim = t.shape[1]
    S = T.sum(axis=0) if len(T) else np.zeros(dim, dtype=object)
    C = T.T.dot(T) if len(T) else np.zeros((dim, dim), dtype=object)
    return np.array([int(x) for x in S], dtype=object), C


def limb_matrices(t):
    """-> (HH, HL, LL) int64 [dim, dim]: t = h * 2^16 + l, h = t >> 16, l = t & 0xffff (exact in int64 up to 2^30 rows)"""
    t = np.ascontiguousarray(t, dtype=np.int64)
    h, l = t >> 16, t & 0xFFFF
    assert (h * 65536 + l == t).all() and h.min(initial=0) >= -65537 and h.max(initial=0) <= 65536
    return h.T @ h, h.T @ l, l.T @ l


def combine(hh, hl, ll):
    """C in Python ints from the limb sums"""
    hh, hl, ll = (np.asarray(x).astype(object) for x in (hh, hl, ll))
    return hh * (1 << 32) + (hl + hl.T) * (1 << 16) + ll


def matrix_from(C, S, n, centered):
    """the f64 matrix of the definition from exact ints"""
    dim = len(S)
    out = np.zeros((dim, dim), dtype=np.float64)
    for d in range(dim):
        for e in range(dim):
            v = int(C[d][e])
            if centered:
                v = n * v - int(S[d]) * int(S[e])
            out[d, e] = float(v) * SCALE
    return out


def moments_reference(rows, centered, part=None, matrix=True):
    """-> (sums int64 [dim], matrix f64 [dim, dim] or None, n)"""
    t, _idx = participating_ints(rows, part)
    n = t.shape[0]
    if not matrix:
        return t.sum(axis=0).astype(np.int64), None, n
    if n * t.shape[1] ** 2 > 2_000_000:  # the limb form, exact in int64 and fast (test_moments_cpu.py checks it against the Python ints)
        S = np.array([int(x) for x in t.sum(axis=0)], dtype=object)
        C = combine(*limb_matrices(t))
    else:
        S, C = exact_moments(t)
    return np.array([int(x) for x in S], dtype=np.int64), matrix_from(C, S, n, centered), n


def f64bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_moments(got, want):
    g_s, g_m, g_n = got
    w_s, w_m, w_n = want
    print("moments: n %d/%d" % (g_n, w_n))
    assert g_n == w_n and g_s.dtype == np.int64
    np.testing.assert_array_equal(g_s, w_s)
    if w_m is None:
        assert g_m is None
    else:
        assert g_m.dtype == np.float64
        np.testing.assert_array_equal(f64bits(g_m), f64bits(w_m))


def rinv_of(rows):
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n2 = canonical_norms(rows)
    has = (n2 >= 2.0 ** -126) & np.isfinite(n2)
    rinv = np.zeros(rows.shape[0], dtype=np.float32)
    rinv[has] = (1.0 / np.sqrt(n2[has])).astype(np.float32)
    return rinv


def project_reference(rows, axes, offsets=None, part=None):
    """-> coords f32 [n, m]: NaN for a row that takes no part"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    axes = np.ascontiguousarray(axes, dtype=np.float32)
    n, m = rows.shape[0], axes.shape[0]
    off = np.zeros(m, dtype=np.float64) if offsets is None else np.asarray(offsets, dtype=np.float64)
    live = takes_part(rows, part)
    rinv = rinv_of(rows).astype(np.float64)
    out = np.full((n, m), np.nan, dtype=np.float32)
    R = rows.astype(np.float64)
    zero = np.zeros((n, 1), dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(m):
            prod = np.concatenate([zero, R * axes[j].astype(np.float64)[None, :]], axis=1)
            a = np.add.accumulate(prod, axis=1)[:, -1]
            c = ((a * rinv) - off[j]).astype(np.float32)
            out[live, j] = c[live]
    return out


def check_project(got, want, ids=None):
    coords, g_ids = got
    print("project: %d x %d" % coords.shape)
    assert coords.dtype == np.float32 and coords.shape == want.shape
    np.testing.assert_array_equal(bits(coords), bits(want) if want.size else np.zeros(want.shape, np.uint32))
    if ids is not None:
        np.testing.assert_array_equal(g_ids, ids)
