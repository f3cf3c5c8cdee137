"""CPU: the host entry points of the corpus moments (pcv_moments_finish, pcv_symmetric_eigen) and the references the GPU tests
use (moments_ref.py).  The finish is compared with Python ints for equality of the f64 bits over the whole 94- to 125-bit range;
the eigen-solver is tested by properties against numpy.linalg.eigh on the same matrix."""
import ctypes as C
import os

import numpy as np
import pytest

import perceive_amd as pa
from moments_ref import SCALE, combine, exact_moments, f64bits, limb_matrices, matrix_from, moments_reference, participating_ints, project_reference
from perceive_amd import _ffi


def finish(hh, hl, ll, sums, n, centered):
    hh, hl, ll = (np.ascontiguousarray(x, dtype=np.int64) for x in (hh, hl, ll))
    dim = hh.shape[0]
    sums = np.ascontiguousarray(sums, dtype=np.int64)
    out = np.full((dim, dim), np.nan, dtype=np.float64)
    _ffi.check(_ffi.lib().pcv_moments_finish(hh.ctypes.data, hl.ctypes.data, ll.ctypes.data, sums.ctypes.data, int(n), dim, centered, out.ctypes.data))
    return out


def want_matrix(hh, hl, ll, sums, n, centered):
    return matrix_from(combine(hh, hl, ll), [int(x) for x in sums], int(n), centered)


# ---- the references themselves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scan_n77_d100", "scan_n1000_d384"])
def test_limb_matrices_reassemble_to_the_python_ints(golden_dir, name):
    rows = np.array(np.load(os.path.join(golden_dir, name + ".npz"))["corpus"], dtype=np.float32)
    t, idx = participating_ints(rows)
    assert len(idx) >= 70 and np.abs(t).max() <= (1 << 32) + (1 << 9)
    C_limbs = combine(*limb_matrices(t))
    cols = np.arange(t.shape[1]) if t.shape[1] <= 100 else np.arange(5, t.shape[1], 24)  # (Python ints are slow: 16 of 384 columns)
    T = t.astype(object)
    C_cols = T.T.dot(T[:, cols])
    assert (C_limbs[:, cols] == C_cols).all() and (C_limbs == C_limbs.T).all()
    # and through the finish: the same bits as float(int) * 2^-64
    hh, hl, ll = limb_matrices(t)
    S = t.sum(axis=0)
    for centered in (0, 1):
        got = finish(hh, hl, ll, S, len(idx), centered)
        np.testing.assert_array_equal(f64bits(got), f64bits(want_matrix(hh, hl, ll, S, len(idx), centered)))
        np.testing.assert_array_equal(f64bits(got), f64bits(moments_reference(rows, centered)[1]))


def test_small_exact_moments_agree_with_limbs():
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((40, 12)).astype(np.float32)
    rows[7] = 0.0
    t, idx = participating_ints(rows)
    assert len(idx) == 39
    S, Cx = exact_moments(t)
    assert (combine(*limb_matrices(t)) == Cx).all()
    assert [int(x) for x in S] == t.sum(axis=0).tolist()


# ---- pcv_moments_finish --------------------------------------------------------------------------------------------------------
def test_finish_random_limb_sums():
    rng = np.random.default_rng(5)
    for dim in (1, 3, 17):
        for _ in range(20):
            n = int(rng.integers(1, 1 << 30))
            hh = rng.integers(-(1 << 62), 1 << 62, size=(dim, dim))
            hh = np.triu(hh) + np.triu(hh, 1).T
            hl = rng.integers(-(1 << 62), 1 << 62, size=(dim, dim))
            ll = rng.integers(0, 1 << 62, size=(dim, dim))
            ll = np.triu(ll) + np.triu(ll, 1).T
            sums = rng.integers(-(1 << 62), 1 << 62, size=dim)
            for centered in (0, 1):
                got = finish(hh, hl, ll, sums, n, centered)
                np.testing.assert_array_equal(f64bits(got), f64bits(want_matrix(hh, hl, ll, sums, n, centered)))
                assert (got == got.T).all()
    # small magnitudes: exact below 2^53
    hh = np.zeros((2, 2), dtype=np.int64)
    ll = np.array([[5, 3], [99, 7]], dtype=np.int64)  # (hh and ll are not read below the diagonal)
    got = finish(ll * 0 + np.tril(ll, -1), hh, ll, [0, 0], 1, 0)
    assert got.tolist() == [[5 * SCALE, 3 * SCALE], [3 * SCALE, 7 * SCALE]]


def test_finish_extremes():
    """n = 2^30 rows with every t = +-2^32 (1 + 2^-23): the largest limb sums the contract allows.  Feature 0 always +, feature 1
    alternating, feature 2 always -."""
    n = 1 << 30
    tp = (1 << 32) + (1 << 9)
    tm = -tp
    hp, lp = tp >> 16, tp & 0xFFFF
    hm, lm = tm >> 16, tm & 0xFFFF
    assert (hp, lp, hm, lm) == (65536, 512, -65537, 65024)
    half = n // 2
    # per feature: (count of +, count of -)
    cnt = [(n, 0), (half, half), (0, n)]
    H = [(hp, lp), (hm, lm)]

    def pair_sum(fa, fb, a_limb, b_limb):
        # features are + or - together in known proportions: f0 +, f2 -, f1 alternates
        total = 0
        for sa in (0, 1):
            for sb in (0, 1):
                # rows where feature a has sign sa and feature b has sign sb
                if fa == fb:
                    c = cnt[fa][sa] if sa == sb else 0
                else:
                    c = {(0, 1): [[half, half], [0, 0]], (0, 2): [[0, n], [0, 0]], (1, 2): [[0, half], [0, half]]}[(min(fa, fb), max(fa, fb))]
                    c = c[sa][sb] if fa < fb else c[sb][sa]
                total += c * H[sa][a_limb] * H[sb][b_limb]
        return total

    hh = np.array([[pair_sum(a, b, 0, 0) for b in range(3)] for a in range(3)], dtype=object)
    hl = np.array([[pair_sum(a, b, 0, 1) for b in range(3)] for a in range(3)], dtype=object)
    ll = np.array([[pair_sum(a, b, 1, 1) for b in range(3)] for a in range(3)], dtype=object)
    S = [n * tp, half * tp + half * tm, n * tm]
    Cx = combine(hh, hl, ll)
    assert int(Cx[0][0]) == n * tp * tp and int(Cx[0][2]) == -n * tp * tp and int(Cx[0][1]) == 0
    assert int(Cx[0][0]).bit_length() == 95 and max(abs(int(x)) for x in hh.ravel()) < 1 << 63
    for centered in (0, 1):
        want = matrix_from(Cx, S, n, centered)
        got = finish(hh.astype(np.int64), hl.astype(np.int64), ll.astype(np.int64), np.array(S, dtype=np.int64), n, centered)
        np.testing.assert_array_equal(f64bits(got), f64bits(want))
    assert (n * int(Cx[1][1])).bit_length() >= 124  # the centred integer of the alternating feature: n C - 0
    assert matrix_from(Cx, S, n, 1)[0, 0] == 0.0 and matrix_from(Cx, S, n, 1)[1, 1] > 0.0


def test_finish_centred_zero_and_ties_to_even():
    # identical rows: n C - S S^T is exactly 0
    t = np.array([[123456789, -987654321, 4294967296]] * 1000, dtype=np.int64)
    hh, hl, ll = limb_matrices(t)
    got = finish(hh, hl, ll, t.sum(axis=0), 1000, 1)
    assert (got == 0.0).all() and not np.signbit(got).any()
    # an integer that is odd at bit 53 with nothing below: a tie, to even.  ll alone carries it.
    z = np.zeros((1, 1), dtype=np.int64)
    for v, want in (((1 << 54) + 2, 1 << 54), ((1 << 54) + 6, (1 << 54) + 8), ((1 << 54) + 3, (1 << 54) + 4), ((1 << 54) + 1, 1 << 54),
                    ((1 << 53) + 1, 1 << 53), ((1 << 53) + 3, (1 << 53) + 4), ((1 << 53) - 1, (1 << 53) - 1)):
        got = finish(z, z, np.array([[v]], dtype=np.int64), [0], 1, 0)
        assert got[0, 0] == float(want) * SCALE == float(v) * SCALE, v
    # negative, through the centring: 1 * 0 - S^2
    got = finish(z, z, z, [(1 << 27) + 1], 1, 1)  # S^2 = 2^54 + 2^28 + 1 -> rounds down to 2^54 + 2^28
    assert got[0, 0] == -float((1 << 54) + (1 << 28)) * SCALE == -float(((1 << 27) + 1) ** 2) * SCALE


def test_host_argument_errors():
    L = _ffi.lib()
    z = np.zeros((2, 2), dtype=np.int64)
    s = np.zeros(2, dtype=np.int64)
    out = np.zeros((2, 2), dtype=np.float64)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert L.pcv_moments_finish(p(z), p(z), p(z), p(s), 1, 2, 0, p(out)) == 0
    assert L.pcv_moments_finish(p(z), p(z), p(z), None, 1, 2, 0, p(out)) == 0  # (the sums are read only when centring)
    assert L.pcv_moments_finish(p(z), p(z), p(z), None, 1, 2, 1, p(out)) == 1
    assert L.pcv_moments_finish(None, p(z), p(z), p(s), 1, 2, 0, p(out)) == 1
    assert L.pcv_moments_finish(p(z), None, p(z), p(s), 1, 2, 0, p(out)) == 1
    assert L.pcv_moments_finish(p(z), p(z), None, p(s), 1, 2, 0, p(out)) == 1
    assert L.pcv_moments_finish(p(z), p(z), p(z), p(s), 1, 2, 0, None) == 1
    assert L.pcv_moments_finish(p(z), p(z), p(z), p(s), 1, 0, 0, p(out)) == 1
    assert L.pcv_moments_finish(p(z), p(z), p(z), p(s), -1, 2, 0, p(out)) == 1
    assert L.pcv_moments_finish(p(z), p(z), p(z), p(s), (1 << 30) + 1, 2, 0, p(out)) == 1
    a = np.eye(2)
    v = np.zeros(2)
    assert L.pcv_symmetric_eigen(p(a), 2, p(v), p(out)) == 0
    assert L.pcv_symmetric_eigen(None, 2, p(v), p(out)) == 1 and L.pcv_symmetric_eigen(p(a), 2, None, p(out)) == 1
    assert L.pcv_symmetric_eigen(p(a), 2, p(v), None) == 1
    assert L.pcv_symmetric_eigen(p(a), 0, p(v), p(out)) == 1 and L.pcv_symmetric_eigen(p(a), 2049, p(v), p(out)) == 1
    for bad in (np.nan, np.inf):
        b = np.array([[1.0, bad], [0.0, 1.0]])
        assert L.pcv_symmetric_eigen(p(b), 2, p(v), p(out)) == 1
        assert "not finite" in L.pcv_last_error().decode()
    b = np.array([[1.0, 0.5], [np.nan, 1.0]])  # below the diagonal: not read
    assert L.pcv_symmetric_eigen(p(b), 2, p(v), p(out)) == 0
    with pytest.raises(ValueError):
        pa.symmetric_eigen(np.zeros((2, 3)))
    # the device entry points: argument errors come before the handle is looked at
    n = C.c_int64()
    assert L.pcv_searcher_moments(None, None, 0, 0, None, None, C.byref(n)) == 1 and "out_sums" in L.pcv_last_error().decode()
    assert L.pcv_searcher_moments(None, None, 0, 0, p(s), None, C.byref(n)) == 1 and "searcher is NULL" in L.pcv_last_error().decode()
    ax = np.zeros((1, 2), dtype=np.float32)
    assert L.pcv_searcher_project(None, p(ax), None, 0, None, 0, 0, None, None, C.byref(n)) == 1 and "m 0" in L.pcv_last_error().decode()
    assert L.pcv_searcher_project(None, p(ax), None, 65, None, 0, 0, None, None, C.byref(n)) == 1
    assert L.pcv_searcher_project(None, p(ax), None, 1, None, 0, 0, None, None, C.byref(n)) == 1 and "searcher is NULL" in L.pcv_last_error().decode()
    assert L.pcv_searcher_principal_axes(None, None, 0, 0, p(ax), p(v), p(v), C.byref(n)) == 1 and "m 0" in L.pcv_last_error().decode()
    assert L.pcv_searcher_last_moment_stats(None, None) == 1 and L.pcv_searcher_last_project_stats(None, None) == 1


# ---- pcv_symmetric_eigen -------------------------------------------------------------------------------------------------------
def eigen_matrices(golden_dir):
    rng = np.random.default_rng(11)
    out = {}
    for n in (1, 2, 3, 100):
        a = rng.standard_normal((n, n))
        out["random%d" % n] = (a + a.T) / 2  # indefinite
    out["diagonal_repeated"] = np.diag([3.0, -1.0, 3.0, 0.0, -1.0, 3.0, 7.0])
    u = rng.standard_normal(40)
    out["rank_one"] = np.outer(u, u)
    out["identity"] = np.eye(5)
    rows = np.array(np.load(os.path.join(golden_dir, "scan_n77_d100.npz"))["corpus"], dtype=np.float32)
    out["golden_covariance"] = moments_reference(rows, 1)[1]
    b = rng.standard_normal((384, 500))
    out["gram384"] = b @ b.T
    return out


def test_symmetric_eigen_properties(golden_dir):
    ratios = {}
    for name, a in eigen_matrices(golden_dir).items():
        n = a.shape[0]
        a = (a + a.T) / 2
        values, vectors = pa.symmetric_eigen(np.triu(a))  # (read from the upper triangle alone)
        assert values.shape == (n,) and vectors.shape == (n, n)
        assert np.abs(vectors @ vectors.T - np.eye(n)).max() <= n * 2.0 ** -50, name
        assert (np.diff(values) <= 0).all(), name
        for v in vectors:  # the sign rule: the component of largest magnitude, the lowest index on ties, is positive
            assert v[int(np.argmax(np.abs(v)))] > 0, name
        fro = np.linalg.norm(a)
        res = np.abs(a @ vectors.T - vectors.T * values[None, :]).max()
        w, V = np.linalg.eigh(a)
        res_np = np.abs(a @ V - V * w[None, :]).max()
        floor = n * 2.0 ** -52 * fro
        ratios[name] = (res / floor if floor else 0.0, res_np / floor if floor else 0.0)
        print("%-18s n %3d residual %.3e numpy %.3e floor %.3e" % (name, n, res, res_np, floor))
        assert res <= max(64 * res_np, floor), name
        np.testing.assert_allclose(values, w[::-1], rtol=0, atol=n * 2.0 ** -50 * max(fro, 1e-300))
    print(ratios)


def test_symmetric_eigen_known_vectors():
    values, vectors = pa.symmetric_eigen(np.array([[2.0, 1.0], [1.0, 2.0]]))
    np.testing.assert_allclose(values, [3.0, 1.0], atol=1e-15)
    r = np.sqrt(0.5)
    np.testing.assert_allclose(vectors, [[r, r], [r, -r]], atol=1e-15)  # ties in magnitude: the lowest index is made positive
    values, vectors = pa.symmetric_eigen(np.array([[-4.0]]))
    assert values.tolist() == [-4.0] and vectors.tolist() == [[1.0]]


def test_project_reference_starts_from_plus_zero():
    rows = np.array([[-1.0, 0.0], [1.0, 1.0]], dtype=np.float32)
    c = project_reference(rows, np.array([[0.0, 1.0]], dtype=np.float32))
    assert not np.signbit(c[0, 0]) and c[0, 0] == 0.0  # (-1 * 0 = -0, and +0 + -0 = +0: what an accumulator that starts at 0 holds)
    assert c[1, 0] == np.float32(np.float64(np.float32(1.0 / np.sqrt(2.0))))
