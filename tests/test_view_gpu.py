"""GPU: views (pcv_searcher_create_view).  Every case compares a view's results with a searcher built fresh from only the allowed
rows (bit for bit: ids, scores, counts, order) and with the oracle over the allowed submatrix, mapped back to ids."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from perceive_amd import _ffi
from perceive_amd.sharded import HIT_DTYPE, merge_topk_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

METRIC = {"cosine": 0, "dot": 1}
PCV_ERR_INVALID = 1
STAGING = pa.search.STAGING_SOURCE


@pytest.fixture(scope="module")
def g1000(golden_dir):
    return np.load(os.path.join(golden_dir, "scan_n1000_d384.npz"))


def queries_256(g1000):
    rng = np.random.default_rng(256)
    return np.concatenate([g1000["queries"], rng.standard_normal((192, 384)).astype(np.float32)])


def build(ctx, dim, metric, parts, screen="auto", mid="off", kernel="auto"):
    """parts = [(source_id, rows, ids), ...] added in this order"""
    s = pa.Searcher(ctx, dim, metric)
    s.set_screening_copy(screen)
    s.set_mid_copy(mid)
    for src, rows, ids in parts:
        if len(rows):
            s.add_rows(src, rows, ids)
    s.finalize()
    s.set_kernel(kernel)
    return s


def allowed_parts(parts, allow):
    """the rows of `parts` whose id is allowed, in the same source and row order (sources without one dropped)"""
    out = []
    for src, rows, ids in parts:
        keep = np.isin(ids, allow)
        if keep.any():
            out.append((src, rows[keep], ids[keep]))
    return out


def assert_same(a, b):
    """(ids, scores, counts) bit for bit"""
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    np.testing.assert_array_equal(a[2], b[2])


def check_oracle(oracle, got, q, parts, k, metric):
    """the oracle's top-k over the allowed submatrix (all sources, in order), mapped back to ids"""
    m = np.concatenate([r for _, r, _ in parts]) if parts else np.zeros((0, q.shape[1]), np.float32)
    ids = np.concatenate([i for _, _, i in parts]) if parts else np.zeros(0, np.int64)
    if m.shape[0] == 0:
        assert (got[2] == 0).all()
        return
    opos, _, ocnt = oracle.topk(q, m, k, METRIC[metric])
    np.testing.assert_array_equal(got[0], np.where(opos >= 0, ids[np.maximum(opos, 0)], -1))
    np.testing.assert_array_equal(got[2], ocnt)


def golden_parts(g1000):
    corpus = g1000["corpus"]
    ids = (np.random.default_rng(7).permutation(1000) * 3 + 11).astype(np.int64)
    return [(1, corpus[:600], ids[:600]), (2, corpus[600:], ids[600:])], ids


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("B", [1, 4, 64, 256])
@pytest.mark.parametrize("kernel", ["auto", "wave", "mfma"])
@pytest.mark.parametrize("screen", ["int8", "bf16", "off"])
def test_golden_parity(ctx, oracle, g1000, screen, kernel, B, metric):
    parts, ids = golden_parts(g1000)
    rng = np.random.default_rng(100 + B)
    pick = rng.choice(ids, 400, replace=False)
    allow = np.concatenate([pick, rng.choice(pick, 50), [-5, 10**12]])  # duplicates, unknown ids
    q = queries_256(g1000)[:B]
    s = build(ctx, 384, metric, parts, screen=screen, kernel=kernel)
    v = s.view(allow)
    sub = allowed_parts(parts, allow)
    f = build(ctx, 384, metric, sub, screen=screen, kernel=kernel)
    assert v.num_rows == 400 and v.source_ids == [1, 2]
    st = v.view_stats()
    assert st["rows"] == 400 and st["ids"] == np.unique(allow).size and st["refreshes"] == 0 and st["build_ms"] > 0
    got = v.search_vectors(None, 10, q)
    assert_same(got, f.search_vectors(None, 10, q))
    check_oracle(oracle, got, q, sub, 10, metric)
    assert v.last_stats()["kernel_used"] == f.last_stats()["kernel_used"]
    assert v.last_stats()["screening_copy"] == f.last_stats()["screening_copy"]
    v.close()
    s.close()
    f.close()


@pytest.mark.parametrize("k", [129, 1000])
@pytest.mark.parametrize("B", [4, 64])
def test_many_results(ctx, oracle, g1000, k, B):
    parts, ids = golden_parts(g1000)
    allow = np.random.default_rng(k).choice(ids, 700, replace=False)
    q = queries_256(g1000)[:B]
    for metric in ("cosine", "dot"):
        s = build(ctx, 384, metric, parts)
        v = s.view(allow)
        sub = allowed_parts(parts, allow)
        f = build(ctx, 384, metric, sub)
        got = v.search_vectors(None, k, q)
        assert_same(got, f.search_vectors(None, k, q))
        check_oracle(oracle, got, q, sub, k, metric)
        assert (got[2] > 128).all()  # (several passes; the oracle fixed the counts)
        v.close()
        s.close()
        f.close()


def test_tie_order(ctx, oracle):
    # rows 100..199 repeat rows 0..99: equal scores, ranked by position; some copies are in the view and some are not
    rng = np.random.default_rng(3)
    base = rng.standard_normal((100, 384)).astype(np.float32)
    m = np.concatenate([base, base, rng.standard_normal((56, 384)).astype(np.float32)])
    ids = np.arange(1000, 1000 + m.shape[0], dtype=np.int64)
    parts = [(1, m, ids)]
    allow = ids[rng.random(m.shape[0]) < 0.6]
    q = np.concatenate([base[:20], rng.standard_normal((12, 384)).astype(np.float32)])
    for screen in ("int8", "off"):
        for metric in ("cosine", "dot"):
            s = build(ctx, 384, metric, parts, screen=screen)
            v = s.view(allow)
            sub = allowed_parts(parts, allow)
            f = build(ctx, 384, metric, sub, screen=screen)
            for k in (5, 150):
                got = v.search_vectors(None, k, q)
                assert_same(got, f.search_vectors(None, k, q))
                check_oracle(oracle, got, q, sub, k, metric)
            v.close()
            s.close()
            f.close()


def test_zero_and_nonfinite_rows(ctx):
    rng = np.random.default_rng(4)
    m = rng.standard_normal((300, 384)).astype(np.float32)
    m[5] = 0.0
    m[6, 3] = np.nan
    m[7, 9] = np.inf
    ids = np.arange(300, dtype=np.int64) + 50
    parts = [(1, m, ids)]
    allow = np.concatenate([ids[:150], ids[5:8]])
    q = rng.standard_normal((16, 384)).astype(np.float32)
    for metric in ("cosine", "dot"):
        s = build(ctx, 384, metric, parts)
        v = s.view(allow)
        f = build(ctx, 384, metric, allowed_parts(parts, allow))
        got = v.search_vectors(None, 200, q)
        assert_same(got, f.search_vectors(None, 200, q))
        bad = {55, 56, 57} if metric == "cosine" else {56, 57}
        assert not (set(got[0].reshape(-1).tolist()) & bad)
        v.close()
        s.close()
        f.close()


def test_source_filters(ctx, oracle, g1000):
    corpus = g1000["corpus"]
    ids = np.arange(1000, dtype=np.int64) + 7
    parts = [(1, corpus[:300], ids[:300]), (3, corpus[300:500], ids[300:500]), (2, corpus[500:800], ids[500:800]),
             (STAGING, corpus[800:], ids[800:])]
    allow = np.concatenate([ids[:300:3], ids[500:800:2], ids[850:900]])  # none of source 3
    q = queries_256(g1000)[:64]
    s = build(ctx, 384, "cosine", parts)
    v = s.view(allow)
    sub = allowed_parts(parts, allow)
    f = build(ctx, 384, "cosine", sub)
    assert v.source_ids == [1, 2] and v.num_rows == 100 + 150  # (staged rows are not counted, as on the parent)
    assert v.view_stats()["rows"] == 300
    assert v.source_num_rows(3) == 0 and v.source_num_rows(STAGING) == 50
    for sources in (None, [1], [3], [2, 3], [], [STAGING], [1, STAGING]):
        for k in (10, 130):
            got = v.search_vectors(sources, k, q)
            assert_same(got, f.search_vectors(sources, k, q))
            want = [p for p in sub if (p[0] != STAGING if sources is None else p[0] in sources)]
            check_oracle(oracle, got, q, want, k, "cosine")
    v.close()
    s.close()
    f.close()


def test_ids_in_several_rows_sources_and_synthetic_rows(ctx, oracle):
    rng = np.random.default_rng(9)
    D = 384
    a = rng.standard_normal((500, D)).astype(np.float32)
    b = rng.standard_normal((400, D)).astype(np.float32)
    a_ids = rng.integers(0, 300, 500).astype(np.int64)  # ids in several rows
    b_ids = rng.integers(200, 600, 400).astype(np.int64)  # ... and in both sources
    for screen in ("int8", "bf16"):
        s = pa.Searcher(ctx, D, "cosine")
        s.set_screening_copy(screen)
        s.add_rows(1, a, a_ids)
        s.add_synthetic(4, 3000, 0xC0FFEE, first_row=100_000, normalize=True)  # implicit ids 100000..102999
        s.add_rows(2, b, b_ids)
        s.finalize()
        syn, syn_ids = s.get_rows(np.arange(500, 3500))
        np.testing.assert_array_equal(syn_ids, np.arange(100_000, 103_000))
        parts = [(1, a, a_ids), (4, syn, syn_ids), (2, b, b_ids)]
        allow = np.concatenate([np.arange(150, 260), rng.choice(np.arange(100_000, 103_500), 900, replace=False)])
        sub = allowed_parts(parts, allow)
        v = s.view(allow)
        f = build(ctx, D, "cosine", sub, screen=screen)
        assert v.num_rows == sum(len(r) for _, r, _ in sub) and v.source_ids == [1, 4, 2]
        q = np.concatenate([syn[::700], rng.standard_normal((60, D)).astype(np.float32)])
        for k in (10, 200):
            got = v.search_vectors(None, k, q)
            assert_same(got, f.search_vectors(None, k, q))
            check_oracle(oracle, got, q, sub, k, "cosine")
        # an empty view, and one of ids that match nothing
        for empty in ([], [-1, 10**15, 99_999]):
            e = s.view(empty)
            assert e.num_rows == 0 and e.source_ids == [] and e.view_stats()["rows"] == 0
            ids, sc, cnt = e.search_vectors(None, 10, q)
            assert (cnt == 0).all() and (ids == -1).all() and np.isnan(sc).all()
            e.close()
        v.close()
        s.close()
        f.close()


def test_staleness(ctx, oracle, g1000):
    parts, ids = golden_parts(g1000)
    rng = np.random.default_rng(12)
    allow = rng.choice(ids, 500, replace=False)
    extra_id = int(allow[0])
    q = queries_256(g1000)[:64]
    s = build(ctx, 384, "cosine", parts)
    v = s.view(np.concatenate([allow, [424242]]))

    def expect(state_parts, hidden=()):
        f = build(ctx, 384, "cosine", allowed_parts(state_parts, np.concatenate([allow, [424242]])))
        if len(hidden):
            f.hide_items(hidden)
        for k in (10, 129):
            assert_same(v.search_vectors(None, k, q), f.search_vectors(None, k, q))
        f.close()

    for _ in range(5):  # the same pass shape again and again: the view's passes are captured into a graph and replayed
        v.search_vectors(None, 10, q)
    expect(parts)
    assert v.view_stats()["refreshes"] == 0  # no parent change: no refresh
    # the parent hides an allowed id
    hid = int(allow[1])
    s.hide_items([hid])
    expect(parts, [hid])
    assert v.view_stats()["refreshes"] == 1
    got = v.search_vectors(None, 1000, q)
    assert hid not in set(got[0].reshape(-1).tolist())
    assert v.view_stats()["refreshes"] == 1
    # ... updates an allowed row
    upd = int(allow[2])
    vec = (3.0 * q[0]).astype(np.float32)
    s.update_items([upd], vec[None])
    parts2 = [(src, r.copy(), i) for src, r, i in parts]
    for _, r, i in parts2:
        r[i == upd] = vec
    expect(parts2, [hid])
    assert v.view_stats()["refreshes"] == 2
    assert v.search_vectors(None, 1, q[:1])[0][0, 0] == upd
    # ... adds and finalizes rows carrying an allowed id (one known, one that matched nothing so far) and one that is not allowed
    new = rng.standard_normal((3, 384)).astype(np.float32)
    s.add_rows(2, new, np.array([extra_id, 424242, 777777], dtype=np.int64))
    assert v.view_stats()["refreshes"] == 2  # (rows added but not finalized: the view still answers the finalized state)
    s.finalize()
    parts3 = parts2[:1] + [(2, np.concatenate([parts2[1][1], new]), np.concatenate([parts2[1][2], [extra_id, 424242, 777777]]))]
    expect(parts3, [hid])
    st = v.view_stats()
    assert st["refreshes"] == 3 and st["rows"] == 502  # (the hidden row stays, unsearchable; two new rows carry allowed ids)
    # ... unhides it again
    s.unhide_items([hid])
    expect(parts3)
    assert v.view_stats()["refreshes"] == 4
    v.close()
    s.close()


def test_parent_runs_as_before(ctx, g1000):
    # two identical parents; one of them has a view that is searched between its own searches: its results and the
    # deterministic parts of its statistics are those of the other
    parts, ids = golden_parts(g1000)
    q = queries_256(g1000)
    a = build(ctx, 384, "cosine", parts)
    b = build(ctx, 384, "cosine", parts)
    v = a.view(ids[::3])
    keys = ("rows_scanned", "scan_launches", "kernel_used", "screening_copy", "bytes_streamed", "mid_copy")
    for step in range(8):
        B = (1, 64, 256, 64)[step % 4]
        k = (10, 10, 10, 200)[step % 4]
        v.search_vectors(None, k, q[:B][::-1].copy())
        ra, sa = a.search_vectors(None, k, q[:B]), a.last_stats()
        rb, sb = b.search_vectors(None, k, q[:B]), b.last_stats()
        assert_same(ra, rb)
        for key in keys:
            assert sa[key] == sb[key], (step, key)
    v.close()
    a.close()
    b.close()


def test_refusals(ctx, g1000):
    parts, ids = golden_parts(g1000)
    s = build(ctx, 384, "cosine", parts)
    v = s.view(ids[:100])
    row = np.zeros((1, 384), np.float32)
    calls = [
        lambda: v.add_rows(1, row, np.array([1], np.int64)),
        lambda: v.add_blobs(1, row.tobytes(), 1, np.array([1], np.int64)),
        lambda: v.add_synthetic(1, 10, 1),
        lambda: v.reserve(1, 10),
        lambda: v.finalize(),
        lambda: v.hide_items([int(ids[0])]),
        lambda: v.unhide_items([int(ids[0])]),
        lambda: v.update_items([int(ids[0])], row),
        lambda: v.update_blobs([int(ids[0])], row.tobytes(), 1),
        lambda: v.set_shard_offset(5),
        lambda: v.set_screening_copy("off"),
        lambda: v.set_mid_copy("on"),
        lambda: v.get_rows([0]),
        lambda: v.rebuild_source([], 1),
    ]
    lib = _ffi.lib()
    for i, call in enumerate(calls):
        with pytest.raises(_ffi.PcvError) as e:
            call()
        assert e.value.status == PCV_ERR_INVALID, i
    assert lib.pcv_searcher_clear_source(v._handle, 1) == PCV_ERR_INVALID
    assert lib.pcv_searcher_replace_source(v._handle, 1, 2) == PCV_ERR_INVALID
    # a view of a view; a parent with rows added but not finalized
    out = C.c_void_p()
    allow = np.arange(3, dtype=np.int64)
    assert lib.pcv_searcher_create_view(v._handle, _ffi.i64p(allow), 3, C.byref(out)) == PCV_ERR_INVALID and not out.value
    s.add_rows(1, row, np.array([5], np.int64))
    assert lib.pcv_searcher_create_view(s._handle, _ffi.i64p(allow), 3, C.byref(out)) == PCV_ERR_INVALID and not out.value
    s.finalize()
    # the view still searches, and its settings are its own
    v.set_kernel("mfma")
    v.set_candidate_capacity(64)
    v.set_tuning(32)
    assert v.search_vectors(None, 3, queries_256(g1000)[:8])[2].tolist() == [3] * 8
    # the parent cannot go while the view is alive
    assert lib.pcv_searcher_destroy(s._handle) == PCV_ERR_INVALID
    assert "view" in lib.pcv_last_error().decode()
    assert s.num_rows == 1001
    assert lib.pcv_searcher_destroy(v._handle) == 0
    v._h = C.c_void_p()
    s.close()


def hits_of(ctx, fn, B, k, extra=0):
    n = (B * k + extra) * HIT_DTYPE.itemsize
    d = ctx.alloc(n)
    try:
        fn(d)
        return ctx.to_host(d, n).view(HIT_DTYPE)
    finally:
        ctx.free(d)


@pytest.mark.parametrize("k", [10, 100])
def test_device_hits_carry_parent_positions(ctx, g1000, k):
    corpus = g1000["corpus"]
    ids = (np.random.default_rng(5).permutation(1000) + 20_000).astype(np.int64)
    pos_of = {int(i): p for p, i in enumerate(ids)}
    allow = np.random.default_rng(6).choice(ids, 450, replace=False)
    q = queries_256(g1000)[:64]
    for metric in ("cosine", "dot"):
        whole = build(ctx, 384, metric, [(1, corpus, ids)])
        wv = whole.view(allow)
        want = wv.search_vectors(None, k, q)
        lists = []
        shards = []
        for lo, hi in ((0, 520), (520, 1000)):
            p = build(ctx, 384, metric, [(1, corpus[lo:hi], ids[lo:hi])])
            p.set_shard_offset(lo)
            pv = p.view(allow)
            h = hits_of(ctx, lambda d: pv.search_device(None, k, q, d), 64, k)
            ok = h["pos"] >= 0
            assert all(pos_of[int(i)] == int(x) for i, x in zip(h["id"][ok], h["pos"][ok]))
            assert ((h["pos"][ok] >= lo) & (h["pos"][ok] < hi)).all()
            hb = hits_of(ctx, lambda d: pv.search_device_begin(None, k, q, d), 64, k, extra=1)
            assert not pv.search_device_end()
            np.testing.assert_array_equal(hb[: 64 * k]["pos"], h["pos"])
            np.testing.assert_array_equal(hb[: 64 * k]["id"], h["id"])
            lists.append(h)
            shards.append((p, pv))
        got = merge_topk_host(metric, 384, np.stack(lists), 2, 64, k)
        assert_same(got, want)
        # the unsharded view's own device list carries the whole corpus's positions
        h = hits_of(ctx, lambda d: wv.search_device(None, k, q, d), 64, k)
        ok = h["pos"] >= 0
        assert all(pos_of[int(i)] == int(x) for i, x in zip(h["id"][ok], h["pos"][ok]))
        for p, pv in shards:
            pv.close()
            p.close()
        wv.close()
        whole.close()


def test_at_size(ctx, oracle):
    # a 1M-id view of 10M synthetic rows (implicit ids = positions), checked against the oracle on sampled queries
    N, D = 10_000_000, 384
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, N, 0xA11, normalize=True)
    s.finalize()
    rng = np.random.default_rng(10)
    allow = np.sort(rng.choice(N, 1_000_000, replace=False)).astype(np.int64)
    v = s.view(allow)
    st = v.view_stats()
    assert st["rows"] == 1_000_000 and st["ids"] == 1_000_000
    sub, sub_ids = s.get_rows(allow)
    np.testing.assert_array_equal(sub_ids, allow)
    q = np.concatenate([sub[rng.choice(1_000_000, 4)], rng.standard_normal((4, D)).astype(np.float32)])
    got = v.search_vectors(None, 10, q)
    check_oracle(oracle, got, q, [(1, sub, sub_ids)], 10, "cosine")
    assert (got[0][:4, 0] == sub_ids[np.argmax(sub @ q[:4].T, axis=0)]).all()
    assert v.last_stats()["rows_scanned"] == 1_000_000
    v.close()
    s.close()


def test_cpp_mirror_views_on_gpu():
    src = os.path.join(ROOT, "tests", "cpp", "view_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "view_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "view_mirror_test: ok" in r.stdout
