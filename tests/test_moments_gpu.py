"""GPU: corpus moments, principal axes and projection (pcv_searcher_moments, _principal_axes, _project), through the Python mirror
of the C ABI.  The reference of every check is moments_ref.py: int64 sums, f64 matrix bits, f32 coordinate bits and ids are compared
for equality.  Each test first asserts on the CPU what makes its input hostile."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from duplicates_ref import bits, build, make_ids
from assign_ref import canonical_norms
from moments_ref import (check_moments, check_project, combine, f64bits, limb_matrices, matrix_from, moments_reference, participating_ints,
                         project_reference, takes_part)
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384
_GOLDEN = {}  # name -> (rows, ids, {centered: reference}): computed once, shared, never changed


def golden(golden_dir, name):
    if name not in _GOLDEN:
        rows = np.ascontiguousarray(np.array(np.load(os.path.join(golden_dir, name + ".npz"))["corpus"], dtype=np.float32))
        ids = make_ids(np.random.default_rng(21), rows.shape[0])
        _GOLDEN[name] = (rows, ids, {c: moments_reference(rows, c) for c in (0, 1)})
    return _GOLDEN[name]


def check_both(s, rows, sources=None, part=None):
    for centered in (0, 1):
        check_moments(s.moments(sources, centered=bool(centered)), moments_reference(rows, centered, part))


def some_axes(rng, m, dim):
    return rng.standard_normal((m, dim)).astype(np.float32)


# ---- 1. golden corpora ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("name", ["scan_n77_d100", "scan_n1000_d384"])
def test_golden(ctx, golden_dir, name, metric):
    rows, ids, want = golden(golden_dir, name)
    n, dim = rows.shape
    s = build(ctx, rows, ids, metric)  # both metrics work on unit rows
    for centered in (0, 1):
        check_moments(s.moments(None, centered=bool(centered)), want[centered])
        st = s.last_moment_stats()
        assert st["rows"] == n and st["participating"] == want[0][2] and st["tile_features"] == 64 and st["row_ranges"] >= 1
        assert st["prep_ms"] > 0 and st["sums_ms"] > 0 and st["syrk_ms"] > 0
    got = s.moments(None, matrix=False)
    check_moments(got, (want[0][0], None, want[0][2]))
    st = s.last_moment_stats()
    assert st["row_ranges"] == 0 and st["syrk_ms"] == 0
    rng = np.random.default_rng(5)
    for m in (1, 7, 8, 9, 64):
        axes = some_axes(rng, m, dim)
        off = rng.standard_normal(m)
        check_project(s.project(None, axes), project_reference(rows, axes), ids)
        check_project(s.project(None, axes, off), project_reference(rows, axes, off), ids)
        st = s.last_project_stats()
        assert st["rows"] == n and st["axes"] == m and st["group"] == (2 if m <= 2 else 8) and st["prep_ms"] > 0 and st["project_ms"] > 0
    s.close()


# ---- 2. block and range edges, dimensions --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [100, 384, 1000])
def test_dimensions(ctx, dim):
    rng = np.random.default_rng(110 + dim)
    n = 150
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids)
    check_both(s, rows)
    axes = some_axes(rng, 9, dim)
    check_project(s.project(None, axes), project_reference(rows, axes), ids)
    s.close()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257, 513])
def test_row_counts(ctx, n):
    """One row, either side of a block (32 rows), either side of the eight blocks of a row range, and more than two ranges."""
    rng = np.random.default_rng(200 + n)
    rows = rng.standard_normal((n, 100)).astype(np.float32)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids)
    check_both(s, rows)
    assert s.last_moment_stats()["row_ranges"] == (n + 255) // 256
    for m in (2, 8):
        axes = some_axes(rng, m, 100)
        check_project(s.project(None, axes), project_reference(rows, axes), ids)
    s.close()


# ---- 3. seven segments ---------------------------------------------------------------------------------------------------------
def test_seven_segments_and_source_lists(ctx):
    rng = np.random.default_rng(31)
    sizes = [64, 96, 32, 1, 128, 5, 300]  # (a piece that is not the last of its source is a whole number of blocks: test_assign_gpu.py)
    src_of = [1, 2, 3, 1, 2, 3, 2]
    n = sum(sizes)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    s = pa.Searcher(ctx, D, "cosine")
    first = np.concatenate([[0], np.cumsum(sizes)])
    where = {1: [], 2: [], 3: []}
    for i, sid in enumerate(src_of):
        s.reserve(sid, sizes[i])
        s.add_rows(sid, rows[first[i] : first[i + 1]], ids[first[i] : first[i + 1]])
        s.finalize()
        where[sid] += list(range(first[i], first[i + 1]))
    assert s.num_segments == 7 and s.num_rows == n

    def rows_of(sources):  # in global position order: by source, in the order the sources were created
        return np.array([r for sid in (1, 2, 3) if sid in sources for r in where[sid]], dtype=np.int64)

    axes = some_axes(rng, 9, D)
    for sources in (None, [1, 2, 3], [3, 1, 2], [2], [3, 1], [1]):
        sel = rows_of([1, 2, 3] if sources is None else sources)
        check_both(s, rows[sel], sources)
        check_project(s.project(sources, axes), project_reference(rows[sel], axes), ids[sel])
    for sources in ([], [99]):
        sums, mat, cnt = s.moments(sources, centered=True)
        assert cnt == 0 and not sums.any() and not mat.any()
        coords, got_ids = s.project(sources, axes)
        assert coords.shape == (0, 9) and got_ids.shape == (0,)
    s.remove_items(ids[where[3]])  # an emptied source selects nothing
    assert s.moments([3])[2] == 0
    sel = rows_of([1, 2])
    check_both(s, rows[sel], None)
    check_project(s.project([2, 3], axes), project_reference(rows[where[2]], axes), ids[where[2]])
    s.close()


# ---- 4. rows that take no part -------------------------------------------------------------------------------------------------
def test_rows_that_take_no_part(ctx):
    rng = np.random.default_rng(71)
    n = 700
    rows = rng.standard_normal((n, D)).astype(np.float32)
    rows[[0, 5]] = 0.0
    edge = list(range(200, 212))  # |x|^2 beside 2^-126: unit rows a little longer and a little shorter than 1, at 2^-63 of their length
    for i, r in enumerate(edge):
        u = rows[r].astype(np.float64)
        rows[r] = (u / np.linalg.norm(u) * (1.0 + (1e-3 if i % 2 else -1e-3)) * 2.0 ** -63).astype(np.float32)
    wild = {300: 2.0 ** -66, 301: 2.0 ** 56}  # |x| near 2^-62 and 2^60: they take part
    for r, sc in wild.items():
        rows[r] = rows[r] * np.float32(sc)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    live = takes_part(rows)
    assert not live[[0, 5]].any() and live[edge].sum() == 6 and (~live[edge]).sum() == 6 and live[list(wild)].all()
    s = build(ctx, rows, ids)
    axes = (some_axes(rng, 9, D) * np.float32(2.0 ** -30)).astype(np.float32)  # (the products with the row of length 2^60 stay finite)
    off = rng.standard_normal(9)
    check_both(s, rows)
    want = project_reference(rows, axes, off)
    assert np.isnan(want[~live]).all() and np.isfinite(want[live]).all()
    check_project(s.project(None, axes, off), want, ids)
    hidden = [1, 20, 21, 150] + list(range(96, 128))  # a whole block among them
    s.hide_items(ids[hidden])
    part = np.ones(n, dtype=bool)
    part[hidden] = False
    check_both(s, rows, part=part)
    want = project_reference(rows, axes, off, part)
    assert np.isnan(want[hidden]).all()
    check_project(s.project(None, axes, off), want, ids)
    s.unhide_items(ids[hidden])
    check_both(s, rows)
    gone = [2, 33, 301, 699]  # rows removed and added again: they come back behind the others
    s.remove_items(ids[gone])
    keep = np.setdiff1d(np.arange(n), gone)
    check_both(s, rows[keep])
    s.add_rows(1, rows[gone], ids[gone])
    s.finalize()
    order = np.concatenate([keep, gone])
    check_both(s, rows[order])
    check_project(s.project(None, axes), project_reference(rows[order], axes), ids[order])
    s.close()
    z = build(ctx, np.zeros((70, D), dtype=np.float32), make_ids(rng, 70))  # no participating row at all
    sums, mat, cnt = z.moments(None, centered=True)
    assert cnt == 0 and not sums.any() and not mat.any()
    assert np.isnan(z.project(None, axes)[0]).all()
    with pytest.raises(pa.PcvError) as e:
        z.principal_axes(None, 2)
    assert e.value.status == 1
    z.close()


# ---- 5. the extremes of the moments kernel -------------------------------------------------------------------------------------
def test_signed_axis_rows_and_a_rinv_that_rounds_up(ctx):
    """Rows +-e_d: t = +-2^32 exactly, h = +-2^16, l = 0.  And rows whose f32 rinv rounds up, so that |t| > 2^32."""
    rng = np.random.default_rng(81)
    dim, n = 64, 300
    rows = np.zeros((n, dim), dtype=np.float32)
    rows[np.arange(n), rng.integers(0, dim, n)] = rng.choice([-1.0, 1.0], size=n) * rng.choice([0.5, 1.0, 4.0], size=n)
    up = []
    for r in range(200, 260):  # one large component and a small one: search for lengths whose 1/|x| rounds up in f32
        rows[r] = 0.0
        rows[r, r % dim] = np.float32(1.0 + rng.random())
        rows[r, (r + 1) % dim] = np.float32(1e-4 * rng.random())
    t, _ = participating_ints(rows)
    up = np.nonzero(np.abs(t).max(axis=1) > (1 << 32))[0]
    print("rows with |t| > 2^32:", len(up), "max |t| - 2^32:", int(np.abs(t).max()) - (1 << 32))
    assert len(up) >= 5 and (np.abs(t[:200]).max(axis=1) == 1 << 32).all()
    assert ((t[:200] >> 16).min() == -65536) and ((t[:200] & 0xFFFF) == 0).all()
    s = build(ctx, rows, make_ids(rng, n))
    check_both(s, rows)
    s.close()


def test_seventy_thousand_copies(ctx):
    """70 000 copies of -e_0: C_00 = 70000 * 2^64 > 2^64, and the centred matrix is exactly 0."""
    dim, n = 64, 70_000
    rows = np.zeros((n, dim), dtype=np.float32)
    rows[:, 0] = -1.0
    s = build(ctx, rows, np.arange(n, dtype=np.int64))
    sums, mat, cnt = s.moments(None, centered=False)
    assert cnt == n and sums[0] == -n * (1 << 32) and not sums[1:].any()
    assert mat[0, 0] == float(n) and np.count_nonzero(mat) == 1
    sums, mat, cnt = s.moments(None, centered=True)
    assert cnt == n and not mat.any() and not np.signbit(mat).any()
    coords, _ = s.project(None, np.eye(2, dim, dtype=np.float32))
    assert (coords[:, 0] == -1.0).all() and (coords[:, 1] == 0.0).all() and not np.signbit(coords[:, 1]).any()
    s.close()


def test_more_than_one_chain(ctx):
    """1 100 000 x 16 rows: more rows than one 2^20-row f64 chain may hold.  The reference: the numpy limb matmuls, exact in int64."""
    rng = np.random.default_rng(91)
    n, dim = 1_100_000, 16
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    t, idx = participating_ints(rows)
    assert len(idx) == n > 1 << 20
    hh, hl, ll = limb_matrices(t)
    S = t.sum(axis=0)
    C = combine(hh, hl, ll)
    s = build(ctx, rows, np.arange(n, dtype=np.int64))
    for centered in (0, 1):
        want = matrix_from(C, [int(x) for x in S], n, centered)
        check_moments(s.moments(None, centered=bool(centered)), (S, want, n))
    assert s.last_moment_stats()["row_ranges"] > 1
    axes = some_axes(rng, 2, dim)
    check_project(s.project(None, axes), project_reference(rows, axes))
    s.close()


# ---- 6. projection against search ----------------------------------------------------------------------------------------------
def test_an_axis_equal_to_a_stored_row(ctx, golden_dir):
    rows, ids, _ = golden(golden_dir, "scan_n1000_d384")
    live = np.nonzero(takes_part(rows))[0]
    n2 = canonical_norms(rows)
    # coord(p) = (x_p . x_r) * rinv_p, so the cosine of p with r is coord(p) / |x_r|.  For p = r it is 1 up to the f32 roundings of rinv
    # and of the coordinate, 2^-24 each: take a row whose reference is well inside the bound
    cand = [int(r) for r in live[:64] if abs(float(project_reference(rows[r : r + 1], rows[r : r + 1])[0, 0]) / np.sqrt(n2[r]) - 1.0) <= 4e-8]
    assert cand
    r = cand[0]
    axis = rows[r : r + 1].copy()
    s = build(ctx, rows, ids)
    want = project_reference(rows, axis)
    coords, got_ids = s.project(None, axis)
    check_project((coords, got_ids), want, ids)
    found, scores, counts = s.search_vectors(None, 5, axis)
    found, scores = np.asarray(found).reshape(-1)[:5], np.asarray(scores).reshape(-1)[:5]
    assert ids[r] in found.tolist()
    pos_of = {int(i): p for p, i in enumerate(ids)}
    for i, sc in zip(found.tolist(), scores.tolist()):
        cos = float(coords[pos_of[i], 0]) / np.sqrt(n2[r])
        print("item %d: cosine %.9f from the coordinate, %.9f from the search" % (i, cos, sc))
        assert abs(cos - sc) <= 1e-7
    # capacity too small, and the report-only form
    n = C.c_int64(-1)
    out = np.zeros((10, 1), dtype=np.float32)
    L = _ffi.lib()
    assert L.pcv_searcher_project(s._handle, _ffi.f32p(axis), None, 1, None, 0, 10, _ffi.f32p(out), None, C.byref(n)) == 1 and n.value == rows.shape[0]
    assert not out.any()
    n = C.c_int64(-1)
    assert L.pcv_searcher_project(s._handle, _ffi.f32p(axis), None, 1, None, 0, 0, None, None, C.byref(n)) == 0 and n.value == rows.shape[0]
    big = np.zeros((rows.shape[0] + 5, 1), dtype=np.float32)
    assert L.pcv_searcher_project(s._handle, _ffi.f32p(axis), None, 1, None, 0, big.shape[0], _ffi.f32p(big), None, C.byref(n)) == 0  # (no ids)
    np.testing.assert_array_equal(bits(big[: rows.shape[0]]), bits(want))
    s.close()


# ---- 7. principal axes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scan_n77_d100", "scan_n1000_d384"])
def test_principal_axes(ctx, golden_dir, name):
    rows, ids, want = golden(golden_dir, name)
    dim = rows.shape[1]
    s = build(ctx, rows, ids)
    m, m_all = 5, min(dim, 64)  # (one call: the eigen-solver is O(dim^3))
    all_axes, all_off, all_var, n = s.principal_axes(None, m_all)
    axes, offsets, variance = all_axes[:m], all_off[:m], all_var[:m]
    sums, cov, n2 = want[1]
    assert n == n2 and axes.shape == (m, dim) and axes.dtype == np.float32 and (np.diff(variance) <= 0).all()
    st = s.last_moment_stats()
    assert st["participating"] == n and st["syrk_ms"] > 0
    # the offsets: the feature-order f64 sum of axis * mean
    mean = sums.astype(np.float64) * 2.0 ** -32 / float(n)
    for j in range(m):
        off = np.add.accumulate(np.concatenate([[0.0], axes[j].astype(np.float64) * mean]))[-1]
        assert off == offsets[j]
    # all the variances sum to trace / n^2
    values, vectors = pa.symmetric_eigen(cov)
    np.testing.assert_array_equal(f64bits(all_var), f64bits(values[: len(all_var)] / (float(n) * float(n))))
    assert abs(values.sum() / float(n) ** 2 - np.trace(cov) / float(n) ** 2) <= dim * 2.0 ** -50
    np.testing.assert_array_equal(bits(axes), bits(vectors[:m].astype(np.float32)))
    # the projected coordinates of the participating rows: mean 0 and the variance of the axis
    coords, got_ids = s.project(None, axes, offsets)
    check_project((coords, got_ids), project_reference(rows, axes, offsets), ids)
    c = coords[takes_part(rows)].astype(np.float64)
    assert c.shape[0] == n
    assert (np.abs(c.mean(axis=0)) <= 2.0 ** -20).all()
    var = (c * c).mean(axis=0) - c.mean(axis=0) ** 2
    print("variance", variance, "of the coordinates", var)
    assert (np.abs(var - variance) <= 1e-5 * variance).all()
    s.close()


# ---- 8. views and search settings ----------------------------------------------------------------------------------------------
def test_views(ctx):
    rng = np.random.default_rng(101)
    n = 600
    rows = rng.standard_normal((n, 128)).astype(np.float32)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids, sources=[(1, 0, 250), (2, 250, 600)])
    allowed = np.nonzero(rng.random(n) < 0.4)[0]
    v = s.view(ids[allowed])
    fresh = build(ctx, rows[allowed], ids[allowed])
    axes = some_axes(rng, 9, 128)
    for centered in (False, True):
        a, b = v.moments(None, centered=centered), fresh.moments(None, centered=centered)
        check_moments(a, b)
        check_moments(a, moments_reference(rows[allowed], int(centered)))
    check_project(v.project(None, axes), project_reference(rows[allowed], axes), ids[allowed])
    assert v.last_moment_stats()["rows"] == len(allowed) and v.last_project_stats()["rows"] == len(allowed)
    in2 = allowed[allowed >= 250]
    check_both(v, rows[in2], [2])
    pa_v, pa_f = v.principal_axes(None, 3), fresh.principal_axes(None, 3)
    for x, y in zip(pa_v[:3], pa_f[:3]):
        np.testing.assert_array_equal(x, y)
    v.close()
    fresh.close()
    s.close()


def test_independent_of_search_settings(ctx):
    rng = np.random.default_rng(91)
    n = 700
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    want = {c: moments_reference(rows, c) for c in (0, 1)}
    axes = some_axes(rng, 9, D)
    want_p = project_reference(rows, axes)
    for copy, kernel, flags, cap in (("off", "auto", 0, None), ("int8", "auto", 32, 64), ("auto", "mfma", 0, 4096), ("auto", "wave", 32, None)):
        s = pa.Searcher(ctx, D, "cosine")
        s.set_screening_copy(copy)
        s.add_rows(1, rows, ids)
        s.finalize()
        s.set_kernel(kernel)
        s.set_tuning(flags)
        if cap:
            s.set_candidate_capacity(cap)
        for c in (0, 1):
            check_moments(s.moments(None, centered=bool(c)), want[c])
        s.search_vectors(None, 5, rows[:3])  # a search in between leaves its pass state behind; the next call does not see it
        check_moments(s.moments(None, centered=True), want[1])
        check_project(s.project(None, axes), want_p, ids)
        s.close()


# ---- 9. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors_on_the_device(ctx):
    rng = np.random.default_rng(3)
    s = build(ctx, rng.standard_normal((40, D)).astype(np.float32), np.arange(40, dtype=np.int64))
    L = _ffi.lib()
    sums = np.zeros(D, dtype=np.int64)
    n = C.c_int64()
    axes = some_axes(rng, 2, D)
    out = np.zeros((40, 2), dtype=np.float32)
    assert L.pcv_searcher_moments(s._handle, None, 0, 0, None, None, C.byref(n)) == 1
    assert L.pcv_searcher_moments(s._handle, None, 0, 0, _ffi.i64p(sums), None, None) == 1
    assert L.pcv_searcher_moments(s._handle, None, 0, 0, _ffi.i64p(sums), None, C.byref(n)) == 0 and n.value == 40

    def proj(m, cap, oc, ax=axes, off=None):
        return L.pcv_searcher_project(s._handle, None if ax is None else _ffi.f32p(ax), None if off is None else off.ctypes.data, m, None, 0, cap,
                                      None if oc is None else _ffi.f32p(oc), None, C.byref(n))

    assert proj(2, 40, out) == 0
    assert proj(0, 40, out) == 1 and proj(65, 40, out) == 1 and proj(2, -1, out) == 1 and proj(2, 40, None) == 1 and proj(2, 39, out) == 1
    assert proj(2, 40, out, ax=None) == 1
    for bad in (np.nan, np.inf, -np.inf):
        ax = axes.copy()
        ax[1, 7] = bad
        assert proj(2, 40, out, ax=ax) == 1 and "not finite" in L.pcv_last_error().decode()
        assert proj(2, 40, out, off=np.array([0.0, bad])) == 1
    ids = np.zeros(40, dtype=np.int64)
    assert L.pcv_searcher_project(s._handle, _ffi.f32p(axes), None, 2, None, 0, 0, None, _ffi.i64p(ids), C.byref(n)) == 1
    v = np.zeros(70, dtype=np.float64)
    big = np.zeros((70, D), dtype=np.float32)

    def paxes(m, a=big, o=v, w=v, cnt=n):
        return L.pcv_searcher_principal_axes(s._handle, None, 0, m, None if a is None else _ffi.f32p(a), None if o is None else o.ctypes.data,
                                             None if w is None else w.ctypes.data, None if cnt is None else C.byref(cnt))

    assert paxes(0) == 1 and paxes(65) == 1 and paxes(2, a=None) == 1 and paxes(2, o=None) == 1 and paxes(2, w=None) == 1 and paxes(2, cnt=None) == 1
    assert L.pcv_searcher_principal_axes(s._handle, _ffi.i64p(ids), 0, 2, _ffi.f32p(big), v.ctypes.data, v.ctypes.data, C.byref(n)) == 1 and n.value == 0
    for bad_m in (0, 65):
        with pytest.raises(ValueError):
            s.principal_axes(None, bad_m)
    with pytest.raises(ValueError):
        s.project(None, np.zeros((2, D + 1), dtype=np.float32))
    with pytest.raises(ValueError):
        s.project(None, axes, np.zeros(3))
    small = build(ctx, rng.standard_normal((40, 8)).astype(np.float32), np.arange(40, dtype=np.int64))
    with pytest.raises(pa.PcvError) as e:  # more axes than dimensions
        small.principal_axes(None, 9)
    assert e.value.status == 1
    assert small.principal_axes(None, 8)[0].shape == (8, 8)
    assert L.pcv_searcher_principal_axes(small._handle, None, 0, 2, _ffi.f32p(big), v.ctypes.data, v.ctypes.data, C.byref(n)) == 0 and n.value == 40
    small.close()
    wide = build(ctx, rng.standard_normal((3, 2052)).astype(np.float32), np.arange(3, dtype=np.int64))
    with pytest.raises(pa.PcvError) as e:
        wide.moments(None)
    assert e.value.status == 3 and "2048" in str(e.value)  # PCV_ERR_UNSUPPORTED
    wide.close()
    s.set_shard_offset(5)  # a sharded searcher
    for call in (lambda: s.moments(None), lambda: s.project(None, axes), lambda: s.principal_axes(None, 2)):
        with pytest.raises(pa.PcvError) as e:
            call()
        assert e.value.status == 1 and "sharded" in str(e.value)
    s.set_shard_offset(0)
    s.add_rows(1, np.ones((1, D), dtype=np.float32), np.array([99], dtype=np.int64))  # pending rows: as a search
    for call in (lambda: s.moments(None), lambda: s.project(None, axes), lambda: s.principal_axes(None, 2)):
        with pytest.raises(pa.PcvError) as e:
            call()
        assert e.value.status == 1
    s.close()


# ---- 10. the C++ mirror --------------------------------------------------------------------------------------------------------
def test_cpp_mirror_moments_program(golden_dir, tmp_path):
    rows, _ids, want = golden(golden_dir, "scan_n77_d100")
    n, dim = rows.shape
    sums, cov, cnt = want[1]
    rng = np.random.default_rng(7)
    axes = some_axes(rng, 3, dim)
    off = rng.standard_normal(3)
    coords = project_reference(rows, axes, off)
    files = {}
    for name, arr, dt in (("rows", rows, "<f4"), ("sums", sums, "<i8"), ("cov", cov, "<f8"), ("axes", axes, "<f4"), ("off", off, "<f8"), ("coords", coords, "<f4")):
        files[name] = str(tmp_path / (name + ".bin"))
        np.ascontiguousarray(arr).astype(dt).tofile(files[name])
    src = os.path.join(ROOT, "tests", "cpp", "moments_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "moments_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    args = [str(n), str(dim), str(cnt), "3"] + [files[k] for k in ("rows", "sums", "cov", "axes", "off", "coords")]
    r = subprocess.run([out] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "moments_mirror_test: ok" in r.stdout
