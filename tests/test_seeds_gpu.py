"""GPU: seed items (pcv_searcher_seeds), through the Python mirror of the C ABI.  The reference of every check is seeds_ref.py: the
oracle's canonical cosine of every participating row with every seed, integer weights by numpy's rint, prefix sums and the draw in
Python ints; ids, positions, the int64 totals, the f32 bits of cover and the count are compared for equality.  Each test first
asserts on the CPU what makes its input hostile."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from duplicates_ref import build, make_ids
from perceive_amd import _ffi
from seeds_ref import METHODS, Reference, bits, check, takes_part, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384
SPAN = 256  # launch rows of one workgroup of the cover kernel (row_jobs.h, kSeedSpanRows)
_GOLDEN = {}  # (name, metric) -> (rows, ids, Reference): computed once, shared, never changed


def golden(oracle, golden_dir, name, metric):
    if (name, metric) not in _GOLDEN:
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        rows = np.array(g["corpus"], dtype=np.float32)
        rng = np.random.default_rng(21)
        if metric == "dot":  # rows of several lengths: the seeds are by cosine all the same
            rows = (rows * rng.uniform(0.5, 1.5, size=(rows.shape[0], 1))).astype(np.float32)
        rows = np.ascontiguousarray(rows)
        ids = make_ids(rng, rows.shape[0])
        _GOLDEN[(name, metric)] = (rows, ids, Reference(oracle, rows, ids))
    return _GOLDEN[(name, metric)]


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)


# ---- 1. golden corpora ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("name", ["scan_n77_d100", "scan_n1000_d384"])
def test_golden(ctx, oracle, golden_dir, name, metric):
    rows, ids, ref = golden(oracle, golden_dir, name, metric)
    n = rows.shape[0]
    P = ref.live.size
    assert P == n or name == "scan_n1000_d384"  # (the larger corpus has rows without a cosine)
    s = build(ctx, rows, ids, metric)
    for method in METHODS:
        for k in (1, 8, 64):
            got = s.seeds(None, k, method, seed=5)
            check(got, ref.seeds(k, method, seed=5))
            assert len(got[0]) == k and got[2][0] == P and len(set(got[1].tolist())) == k
            st = s.last_seed_stats()
            assert st["rows"] == n and st["participating"] == P and st["steps"] == k and st["method"] == {"farthest": 0, "kmeans++": 1}[method]
            assert st["prep_ms"] > 0 and st["steps_ms"] > 0
    s.close()


# ---- 2. span and block edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 1])
def test_span_and_block_edges(ctx, oracle, n):
    """A workgroup's span is 256 launch rows: one row, either side of a block, either side of a span, and three spans with one
    row in the last."""
    assert SPAN == 256
    rng = np.random.default_rng(200 + n)
    rows = rng.standard_normal((n, 64)).astype(np.float32)
    ids = make_ids(rng, n)
    ref = Reference(oracle, rows, ids)
    k = min(8, n)
    s = build(ctx, rows, ids)
    for method in METHODS:
        for seed in (0, 1, 2):
            got = s.seeds(None, k, method, seed)
            check(got, ref.seeds(k, method, seed))
            assert len(got[0]) == k
    # the last row, alone in its span when n = 2 * SPAN + 1, as the first seed and as the farthest row
    got = s.seeds(None, k, "farthest", first_id=int(ids[n - 1]))
    check(got, ref.seeds(k, "farthest", first_id=int(ids[n - 1])))
    assert got[1][0] == n - 1
    s.close()


# ---- 3. seven segments ---------------------------------------------------------------------------------------------------------
def test_seven_segments_and_source_lists(ctx, oracle):
    rng = np.random.default_rng(31)
    sizes = [64, 96, 32, 1, 128, 5, 300]  # (a piece that is not the last of its source is a whole number of blocks: test_assign_gpu.py)
    src_of = [1, 2, 3, 1, 2, 3, 2]
    n, k = sum(sizes), 12
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
    # launch rows have gaps behind the segments of 1, 5 and 300 rows (their last blocks are not full)
    assert [sz % 32 for sz in sizes] == [0, 0, 0, 1, 0, 5, 12]

    def rows_of(sources):  # in global position order: by source, in the order the sources were created
        return np.array([r for sid in (1, 2, 3) if sid in sources for r in where[sid]], dtype=np.int64)

    order = rows_of([1, 2, 3])
    pos_of = np.empty(n, dtype=np.int64)
    pos_of[order] = np.arange(n)

    def want(sources, method, seed):
        sel = rows_of(sources)
        return Reference(oracle, rows[sel], ids[sel], positions=pos_of[sel]).seeds(k, method, seed)

    for sources in (None, [1, 2, 3], [3, 1, 2], [2], [3, 1], [1]):
        for method in METHODS:
            got = s.seeds(sources, k, method, seed=9)
            check(got, want([1, 2, 3] if sources is None else sources, method, 9))
            np.testing.assert_array_equal(ids[order[got[1]]], got[0])  # the positions are global ones
    for sources in ([], [99]):
        assert all(len(x) == 0 for x in s.seeds(sources, k))
    # a source emptied by remove_items: its rows are gone, and it selects nothing
    s.remove_items(ids[where[3]])
    assert all(len(x) == 0 for x in s.seeds([3], k))
    where[3] = []
    order = rows_of([1, 2])
    pos_of[order] = np.arange(len(order))
    for sources, sel in ((None, [1, 2]), ([2, 3], [2])):
        check(s.seeds(sources, k, "kmeans++", 4), want(sel, "kmeans++", 4))
    s.close()


# ---- 4. prefix boundaries ------------------------------------------------------------------------------------------------------
def test_prefix_boundaries_on_an_orthonormal_corpus(ctx, oracle):
    """600 signed unit vectors of a 640-d space: every cosine between two rows is exactly 0, so every uncovered row weighs 2^32
    exactly, T_j = (P - j) * 2^32, and the draw t falls on a boundary of the prefix sums whenever its low 32 bits are 0 — and just
    below or above one all the time.  Seeds 0 .. 95: with 0 .. 63 the reference picks the first row of spans 0 and 1 but no last row
    of a span; seed 95 picks row 255."""
    rng = np.random.default_rng(41)
    n, dim, k = 600, 640, 8
    axes = rng.permutation(dim)[:n]
    rows = np.zeros((n, dim), dtype=np.float32)
    rows[np.arange(n), axes] = rng.choice([-1.0, 1.0], size=n)
    ids = make_ids(rng, n)
    ref = Reference(oracle, rows, ids)
    seeds = range(96)
    wants = [ref.seeds(k, "kmeans++", seed) for seed in seeds]
    picked = np.concatenate([w[1] for w in wants])
    for w in wants:
        assert w[2].tolist() == [n] + [(n - j) << 32 for j in range(1, k)] and (w[3][1:] == 0).all()
    first_rows = {int(p) // SPAN for p in picked if p % SPAN == 0}
    last_rows = {int(p) // SPAN for p in picked if p % SPAN == SPAN - 1}
    print("first rows of spans", sorted(first_rows), "last rows of spans", sorted(last_rows), "spans", sorted({int(p) // SPAN for p in picked}))
    assert first_rows and last_rows and len({int(p) // SPAN for p in picked}) >= 2
    s = build(ctx, rows, ids)
    for seed, w in zip(seeds, wants):
        check(s.seeds(None, k, "kmeans++", seed), w)
    # farthest first on all ties: positions 0, 1, 2, ...
    got = s.seeds(None, k, "farthest")
    check(got, ref.seeds(k, "farthest"))
    assert got[1].tolist() == list(range(k))
    s.close()


# ---- 5. ties under the farthest rule -------------------------------------------------------------------------------------------
def test_farthest_ties(ctx, oracle):
    """Row 0 is e0 and is the first seed.  A family of rows -e0 + d e1, d a few f32 ulps apart around 0.01, lies opposite to it:
    their cosines with the seed differ by up to 1e-10 and more, but rint(. * 2^32) makes runs of them equal — the farthest row is the
    one of the heaviest run stored first, not the one with the smallest cosine.  Then groups of 16 identical rows: the lower position."""
    rng = np.random.default_rng(51)
    n, dim = 400, 64
    rows = np.abs(rng.standard_normal((n, dim))).astype(np.float32)  # the others: in the seed's half space
    rows[0] = 0.0
    rows[0, 0] = 1.0
    fam = np.arange(60, 100)
    d = np.float32(0.01)
    for i, r in enumerate(fam):  # stored with d descending: the smallest cosine comes last
        rows[r] = 0.0
        rows[r, 0] = -1.0
        rows[r, 1] = d + np.float32(7 + len(fam) - 1 - i) * np.spacing(d)  # (from 7 ulps on: the heaviest run is a full one)
    groups = []
    spots = rng.permutation(np.arange(100, n))
    for gi in range(2):  # (disjoint)
        members = np.sort(spots[16 * gi : 16 * gi + 16])
        rows[members] = rng.standard_normal(dim).astype(np.float32)
        groups.append(members)
    ids = make_ids(rng, n)
    ref = Reference(oracle, rows, ids)
    c = ref.column(0)
    w = weights(c)
    top = np.nonzero(w == w.max())[0]
    print("heaviest run: %d rows, cosines %.3e apart; smallest cosine at %d, pick %d" % (len(top), c[top].max() - c[top].min(), int(np.argmin(c)), int(top[0])))
    assert len(top) >= 4 and set(top.tolist()) <= set(fam.tolist()) and c[top].max() - c[top].min() >= 1e-10
    assert int(np.argmin(c)) == fam[-1] and top[0] != fam[-1] and len(set(c[top].tolist())) == len(top)
    s = build(ctx, rows, ids)
    k = 40
    got = s.seeds(None, k, "farthest")
    want = ref.seeds(k, "farthest")
    check(got, want)
    assert got[1][0] == 0 and got[1][1] == top[0]
    for members in groups:  # of a group of identical rows only the one stored first can be picked
        assert not np.isin(got[1], members[1:]).any()
        if np.isin(got[1], members).any():
            assert members[0] in got[1]
    check(s.seeds(None, k, "kmeans++", 2), ref.seeds(k, "kmeans++", 2))
    s.close()


# ---- 6. early stop -------------------------------------------------------------------------------------------------------------
def test_early_stop(ctx, oracle):
    rng = np.random.default_rng(61)
    v = rng.standard_normal(D).astype(np.float32)
    rows = np.ascontiguousarray(np.stack([v * np.float32(2.0 ** (i % 7 - 3)) for i in range(200)]))
    ids = make_ids(rng, 200)
    ref = Reference(oracle, rows, ids)
    assert (weights(ref.column(0)) == 0).all()  # T_1 == 0: every row points the way of the first seed
    s = build(ctx, rows, ids)
    for method in METHODS:
        got = s.seeds(None, 5, method, 1)
        check(got, ref.seeds(5, method, 1))
        assert len(got[0]) == 1 and got[2].tolist() == [200]
        assert s.last_seed_stats()["steps"] == 1
    with pytest.raises(ValueError):  # kmeans cannot start from one seed of five
        s.kmeans(None, 5, "kmeans++")
    s.close()
    # k larger than the number of participating rows
    rows = rng.standard_normal((40, D)).astype(np.float32)
    rows[[3, 17]] = 0.0
    ids = make_ids(rng, 40)
    ref = Reference(oracle, rows, ids)
    assert ref.live.size == 38
    s = build(ctx, rows, ids)
    for method in METHODS:
        got = s.seeds(None, 64, method, 8)
        check(got, ref.seeds(64, method, 8))
        assert len(got[0]) == 38 and sorted(got[1].tolist()) == ref.live.tolist()
    # a selection with no participating row
    s.hide_items(ids)
    assert all(len(x) == 0 for x in s.seeds(None, 4))
    st = s.last_seed_stats()
    assert st["rows"] == 40 and st["participating"] == 0 and st["steps"] == 0
    s.close()
    z = build(ctx, np.zeros((70, D), dtype=np.float32), make_ids(rng, 70))
    assert all(len(x) == 0 for x in z.seeds(None, 4, "farthest"))
    z.close()


# ---- 7. rows that take no part -------------------------------------------------------------------------------------------------
def test_rows_that_take_no_part(ctx, oracle):
    rng = np.random.default_rng(71)
    n, k = 700, 24
    rows = rng.standard_normal((n, D)).astype(np.float32)
    rows[[0, 5]] = 0.0  # (the first row among them: step 0 of the farthest rule starts at row 1)
    edge = list(range(200, 212))  # |x|^2 beside 2^-126: unit rows a little longer and a little shorter than 1, at 2^-63 of their length
    for i, r in enumerate(edge):
        u = rows[r].astype(np.float64)
        rows[r] = (u / np.linalg.norm(u) * (1.0 + (1e-3 if i % 2 else -1e-3)) * 2.0 ** -63).astype(np.float32)
    wild = {300: 2.0 ** -66, 301: 2.0 ** 56, 500: 2.0 ** -66, 501: 2.0 ** 56}  # |x| near 2^-62 and 2^60: they take part
    for r, sc in wild.items():
        rows[r] = rows[r] * np.float32(sc)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, n)
    live = takes_part(rows)
    assert not live[[0, 5]].any() and live[edge].sum() == 6 and (~live[edge]).sum() == 6 and live[list(wild)].all()
    n2 = (rows[list(wild)].astype(np.float64) ** 2).sum(axis=1)
    assert ((n2 < 2.0 ** -40) | (n2 > 2.0 ** 40)).all()
    s = build(ctx, rows, ids)
    ref = Reference(oracle, rows, ids)
    picked = set()
    for method in METHODS:
        for seed in range(4):
            got = s.seeds(None, k, method, seed)
            check(got, ref.seeds(k, method, seed))
            assert live[got[1]].all()
            picked |= set(got[1].tolist())
    assert s.seeds(None, 1, "farthest")[1].tolist() == [1]
    for r in wild:  # a wild row as the centre of a cover step
        check(s.seeds(None, 6, "kmeans++", 3, first_id=int(ids[r])), ref.seeds(6, "kmeans++", 3, first_id=int(ids[r])))
    # hidden rows, a whole block among them
    hidden = [1, 20, 21, 150] + list(range(96, 128))
    s.hide_items(ids[hidden])
    part = np.ones(n, dtype=bool)
    part[hidden] = False
    href = Reference(oracle, rows, ids, part)
    for method in METHODS:
        got = s.seeds(None, k, method, 6)
        check(got, href.seeds(k, method, 6))
        assert not np.isin(got[1], hidden).any()
    assert s.seeds(None, 1, "farthest")[1].tolist() == [2]
    s.unhide_items(ids[hidden])
    check(s.seeds(None, k, "kmeans++", 6), ref.seeds(k, "kmeans++", 6))
    # rows removed and added again: they come back behind the others
    gone = [2, 33, 301, 699]
    s.remove_items(ids[gone])
    keep = np.setdiff1d(np.arange(n), gone)
    check(s.seeds(None, k, "kmeans++", 7), Reference(oracle, rows[keep], ids[keep]).seeds(k, "kmeans++", 7))
    s.add_rows(1, rows[gone], ids[gone])
    s.finalize()
    order = np.concatenate([keep, gone])
    back = Reference(oracle, rows[order], ids[order])
    for method in METHODS:
        check(s.seeds(None, k, method, 7), back.seeds(k, method, 7))
    got = s.seeds(None, 3, "farthest", first_id=int(ids[699]))
    check(got, back.seeds(3, "farthest", first_id=int(ids[699])))
    assert got[1][0] == n - 1
    s.close()


# ---- 8. first_id ---------------------------------------------------------------------------------------------------------------
def test_first_id(ctx, oracle):
    rng = np.random.default_rng(81)
    n, k = 300, 6
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    ids[270] = ids[40]   # carried by two rows: the first by position is used
    ids[10] = ids[150]   # ... and here the first one has no cosine: the second is the first PARTICIPATING one
    rows[10] = 0.0
    s = build(ctx, rows, ids)
    only_hidden = int(ids[99])
    s.hide_items(np.array([only_hidden], dtype=np.int64))
    part = np.ones(n, dtype=bool)
    part[99] = False
    ref = Reference(oracle, rows, ids, part)
    for method in METHODS:
        got = s.seeds(None, k, method, 11, first_id=int(ids[40]))
        check(got, ref.seeds(k, method, 11, first_id=int(ids[40])))
        assert got[1][0] == 40 and got[0][0] == ids[40]
        got = s.seeds(None, k, method, 11, first_id=int(ids[150]))
        check(got, ref.seeds(k, method, 11, first_id=int(ids[150])))
        assert got[1][0] == 150
    unknown = int(ids.max()) + 1
    out_ids = np.full(k, -77, dtype=np.int64)
    out_pos = np.full(k, -77, dtype=np.int64)
    out_tot = np.full(k, -77, dtype=np.int64)
    out_cov = np.full(k, -77, dtype=np.float32)
    count = C.c_int32(-5)
    for bad in (only_hidden, unknown):
        with pytest.raises(ValueError):
            ref.seeds(k, "kmeans++", 0, first_id=bad)
        for method in (0, 1):
            first = np.array([bad], dtype=np.int64)
            status = _ffi.lib().pcv_searcher_seeds(s._handle, None, 0, k, method, 0, _ffi.i64p(first), _ffi.i64p(out_ids), _ffi.i64p(out_pos),
                                                   _ffi.i64p(out_tot), _ffi.f32p(out_cov), C.byref(count))
            assert status == 1 and "first_id %d" % bad in _ffi.lib().pcv_last_error().decode()  # PCV_ERR_INVALID
            assert count.value == -5 and (out_ids == -77).all() and (out_pos == -77).all() and (out_tot == -77).all() and (out_cov == -77).all()
        with pytest.raises(pa.PcvError) as e:
            s.seeds(None, k, first_id=bad)
        assert e.value.status == 1
    with pytest.raises(pa.PcvError):  # nothing selected: nobody carries it
        s.seeds([], k, first_id=int(ids[40]))
    # unused slots of a call that stops early: -1 / -1 / 0 / NaN
    few = build(ctx, np.ones((5, D), dtype=np.float32), np.arange(5, dtype=np.int64))
    status = _ffi.lib().pcv_searcher_seeds(few._handle, None, 0, k, 0, 0, None, _ffi.i64p(out_ids), _ffi.i64p(out_pos), _ffi.i64p(out_tot),
                                           _ffi.f32p(out_cov), C.byref(count))
    assert status == 0 and count.value == 1
    assert out_ids.tolist() == [0] + [-1] * (k - 1) and out_pos.tolist() == [0] + [-1] * (k - 1) and out_tot.tolist() == [5] + [0] * (k - 1)
    assert np.isnan(out_cov).all()
    few.close()
    s.close()


def test_a_call_that_fails_behind_its_kernels_leaves_the_searcher_as_it_was(ctx, oracle):
    """An unknown first_id is found out on the device: the call fails with every kernel run and its buffers still to give back.  The
    calls after it — seeds again, and a search — give what they gave before, byte for byte."""
    rng = np.random.default_rng(82)
    n, d, k = 200, 32, 4
    rows = rng.standard_normal((n, d)).astype(np.float32)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids, sources=[(1, 0, 120), (2, 120, n)])
    assert s.num_segments == 2
    q = rows[:3] + np.float32(0.25) * rng.standard_normal((3, d)).astype(np.float32)
    hits = s.search_vectors(None, 5, q)
    first = s.seeds(None, k)
    check(first, Reference(oracle, rows, ids).seeds(k, "kmeans++"))
    unknown = int(ids.max()) + 1
    assert unknown not in set(ids.tolist())
    with pytest.raises(pa.PcvError) as e:
        s.seeds(None, k, first_id=unknown)
    assert e.value.status == 1  # PCV_ERR_INVALID
    assert "seeds: no participating row of the selected sources carries first_id %d" % unknown in str(e.value)
    same(s.seeds(None, k), first)
    same(s.search_vectors(None, 5, q), hits)
    s.close()


# ---- 9. independence of the search settings ------------------------------------------------------------------------------------
def test_independent_of_search_settings(ctx, oracle):
    rng = np.random.default_rng(91)
    n, k = 700, 16
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    ref = Reference(oracle, rows, ids)
    want = {m: ref.seeds(k, m, 13) for m in METHODS}
    for copy, kernel, flags, cap in (("off", "auto", 0, None), ("int8", "auto", 32, 64), ("auto", "mfma", 0, 4096), ("auto", "wave", 32, None)):
        s = pa.Searcher(ctx, D, "cosine")
        s.set_screening_copy(copy)
        s.add_rows(1, rows, ids)
        s.finalize()
        s.set_kernel(kernel)
        s.set_tuning(flags)
        if cap:
            s.set_candidate_capacity(cap)
        for m in METHODS:
            check(s.seeds(None, k, m, 13), want[m])
        s.search_vectors(None, 5, rows[:3])  # a search in between leaves its pass state behind; the next call does not see it
        for m in METHODS:
            check(s.seeds(None, k, m, 13), want[m])
            same(s.seeds(None, k, m, 13), s.seeds(None, k, m, 13))
        s.close()


# ---- 10. views -----------------------------------------------------------------------------------------------------------------
def test_views(ctx, oracle):
    rng = np.random.default_rng(101)
    n, k = 600, 10
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    s = build(ctx, rows, ids, sources=[(1, 0, 250), (2, 250, 600)])
    allowed = np.nonzero(rng.random(n) < 0.4)[0]  # ascending: the parent's order
    v = s.view(ids[allowed])
    fresh = build(ctx, rows[allowed], ids[allowed])
    ref = Reference(oracle, rows[allowed], ids[allowed])
    for m in METHODS:
        a, b = v.seeds(None, k, m, 17), fresh.seeds(None, k, m, 17)
        np.testing.assert_array_equal(a[0], b[0])
        check(a, ref.seeds(k, m, 17))
        np.testing.assert_array_equal(ids[allowed[a[1]]], a[0])  # a view numbers its rows from 0, in its parent's order
    assert v.last_seed_stats()["rows"] == len(allowed)
    in2 = allowed[allowed >= 250]
    got = v.seeds([2], k, "farthest")
    check(got, Reference(oracle, rows[in2], ids[in2], positions=np.arange(len(allowed))[allowed >= 250]).seeds(k, "farthest"))
    v.close()
    fresh.close()
    s.close()


# ---- 11. dimensions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [100, 384, 768, 1000])
def test_dimensions(ctx, oracle, dim):
    rng = np.random.default_rng(110 + dim)
    n, k = 300, 8
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    ids = make_ids(rng, n)
    ref = Reference(oracle, rows, ids)
    s = build(ctx, rows, ids)
    for m in METHODS:
        check(s.seeds(None, k, m, dim), ref.seeds(k, m, dim))
    s.close()


# ---- 12. kmeans ----------------------------------------------------------------------------------------------------------------
def test_kmeans_seeds_itself(ctx, oracle, golden_dir):
    rows, ids, ref = golden(oracle, golden_dir, "scan_n1000_d384", "cosine")
    assert len(set(ids.tolist())) == len(ids)
    s = build(ctx, rows, ids)
    k = 8
    for m in METHODS:
        picked = s.seeds(None, k, m, seed=3)[0]
        np.testing.assert_array_equal(picked, ref.seeds(k, m, 3)[0])
        a = s.kmeans(None, k, m, max_iters=5, seed=3)
        b = s.kmeans(None, k, picked, max_iters=5)
        assert len(a) == len(b) == 7
        for x, y in zip(a, b):
            if isinstance(x, np.ndarray):
                np.testing.assert_array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
            else:
                assert x == y
        assert a[3].shape == (len(ids),) and a[0].shape == (k, rows.shape[1])
    with pytest.raises(ValueError):
        s.kmeans(None, k, "random")
    s.close()


# ---- 13. argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors_on_the_device(ctx):
    s = build(ctx, np.ones((40, D), dtype=np.float32), np.arange(40, dtype=np.int64))
    out = [np.zeros(8, dtype=np.int64) for _ in range(3)] + [np.zeros(8, dtype=np.float32)]
    count = C.c_int32()

    def raw(k, method):
        return _ffi.lib().pcv_searcher_seeds(s._handle, None, 0, k, method, 0, None, _ffi.i64p(out[0]), _ffi.i64p(out[1]), _ffi.i64p(out[2]),
                                             _ffi.f32p(out[3]), C.byref(count))

    assert raw(0, 1) == 1 and raw(pa.search.PCV_MAX_SEEDS + 1, 1) == 1 and raw(3, 2) == 1 and raw(3, 1) == 0
    for k in (0, pa.search.PCV_MAX_SEEDS + 1):
        with pytest.raises(ValueError):
            s.seeds(None, k)
    with pytest.raises(ValueError):
        s.seeds(None, 3, method=2)
    s.set_shard_offset(5)  # a sharded searcher
    with pytest.raises(pa.PcvError) as e:
        s.seeds(None, 3)
    assert e.value.status == 1 and "sharded" in str(e.value)
    s.set_shard_offset(0)
    assert len(s.seeds(None, 3)[0]) == 1  # (identical rows: one seed covers them)
    s.add_rows(1, np.ones((1, D), dtype=np.float32), np.array([99], dtype=np.int64))  # pending rows: as a search
    with pytest.raises(pa.PcvError) as e:
        s.seeds(None, 3)
    assert e.value.status == 1
    s.close()


# ---- 14. the C++ mirror --------------------------------------------------------------------------------------------------------
def test_cpp_mirror_seeds_program(oracle, golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "scan_n77_d100.npz"))
    rows = np.ascontiguousarray(np.array(g["corpus"], dtype=np.float32))
    n, dim = rows.shape
    ids = 5000 + 3 * np.arange(n, dtype=np.int64)
    k, seed = 8, 12345
    want = Reference(oracle, rows, ids).seeds(k, "kmeans++", seed)
    assert len(want[0]) == k
    raw = tmp_path / "rows.f32"
    rows.astype("<f4").tofile(str(raw))
    args = [str(raw), str(n), str(dim), str(k), "1", str(seed), str(k)]
    for j in range(k):
        args += [str(int(want[0][j])), str(int(want[1][j])), str(int(want[2][j])), "%08x" % int(bits(want[3][j : j + 1])[0])]
    src = os.path.join(ROOT, "tests", "cpp", "seeds_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "seeds_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "seeds_mirror_test: ok" in r.stdout
