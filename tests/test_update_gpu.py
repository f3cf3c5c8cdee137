"""GPU: updated items (pcv_searcher_update_rows).  The reference results come from the oracle over the UPDATED matrix and from a
second searcher built fresh from it: after an update every search returns bit for bit what the fresh searcher returns."""
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

METRIC = {"cosine": 0, "dot": 1}
PCV_ERR_INVALID = 1


@pytest.fixture(scope="module")
def g1000(golden_dir):
    return np.load(os.path.join(golden_dir, "scan_n1000_d384.npz"))


def queries_256(g1000):
    rng = np.random.default_rng(256)
    return np.concatenate([g1000["queries"], rng.standard_normal((192, 384)).astype(np.float32)])


def fresh(ctx, dim, metric, parts, screen="auto", mid="off", kernel="auto"):
    """A searcher built from scratch: parts = [(source_id, rows, ids or None), ...] in this order."""
    s = pa.Searcher(ctx, dim, metric)
    s.set_screening_copy(screen)
    s.set_mid_copy(mid)
    for src, rows, ids in parts:
        s.add_rows(src, rows, ids)
    s.finalize()
    s.set_kernel(kernel)
    return s


def assert_same(a, b):
    """(ids, scores, counts) bit for bit"""
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    np.testing.assert_array_equal(a[2], b[2])


def new_vectors(rng, n, d, spread=(0.5, 3.0)):
    return (rng.standard_normal((n, d)) * rng.uniform(*spread, (n, 1))).astype(np.float32)


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("B", [1, 4, 64, 256])
@pytest.mark.parametrize("kernel", ["auto", "wave", "mfma"])
@pytest.mark.parametrize("screen", ["int8", "bf16", "off"])
def test_golden_parity(ctx, oracle, g1000, screen, kernel, B, metric):
    corpus = g1000["corpus"]
    q = queries_256(g1000)[:B]
    s = fresh(ctx, 384, metric, [(1, corpus, None)], screen=screen, kernel=kernel)  # ids = positions
    top, _, _ = s.search_vectors(None, 3, q)
    rng = np.random.default_rng(1000 + B)
    upd = np.unique(np.concatenate([top.reshape(-1), rng.choice(1000, 50, replace=False)]))
    vecs = new_vectors(rng, upd.size, 384)
    found, changed = s.update_items(upd, vecs)
    assert found.all() and changed == upd.size
    assert s.num_rows == 1000 and s.source_num_rows(1) == 1000
    m = corpus.copy()
    m[upd] = vecs
    f = fresh(ctx, 384, metric, [(1, m, None)], screen=screen, kernel=kernel)
    for k in (10, 200):
        got = s.search_vectors(None, k, q)
        assert_same(got, f.search_vectors(None, k, q))
        opos, _, ocnt = oracle.topk(q, m, k, METRIC[metric])
        np.testing.assert_array_equal(got[0], opos)
        np.testing.assert_array_equal(got[2], ocnt)
    rows, rid = s.get_rows(upd)
    np.testing.assert_array_equal(rows, vecs)
    np.testing.assert_array_equal(rid, upd)
    s.close()
    f.close()


@pytest.mark.parametrize("mid", ["off", "on"])
def test_spike_into_a_gaussian_block(ctx, oracle, mid):
    # Block 0 (rows 0..31) holds small Gaussian rows: its int8 s_blk is far above 127 / 0.99.  Row 5 becomes a spike (one component
    # ~0.99 of its norm): re-quantised with the old s_blk it would clip and the coarse screen would drop it behind its near copies
    # in block 1.  The whole block is re-packed: it is the top hit of a query equal to it, with cosine 1.
    rng = np.random.default_rng(5)
    D = 384
    m = (0.01 * rng.standard_normal((64, D))).astype(np.float32)
    spike = (0.0005 * rng.standard_normal(D)).astype(np.float32)
    spike[0] = 0.9
    m[32:38] = spike + 0.005 * rng.standard_normal((6, D)).astype(np.float32)  # near copies (cos ~0.99) raise the threshold
    s = fresh(ctx, D, "cosine", [(1, m, np.arange(64, dtype=np.int64))], screen="int8", mid=mid, kernel="mfma")
    q = np.concatenate([spike[None], rng.standard_normal((7, D)).astype(np.float32)])
    found, changed = s.update_items([5], spike[None])
    assert found.all() and changed == 1
    ids, sc, _ = s.search_vectors(None, 5, q)
    st = s.last_stats()
    assert st["kernel_used"] == 2 and st["screening_copy"] == 2 and st["mid_copy"] == (1 if mid == "on" else 0)
    assert ids[0, 0] == 5 and set(ids[0, 1:]) <= set(range(32, 38))
    assert abs(sc[0, 0] - 1.0) <= 1e-7
    m2 = m.copy()
    m2[5] = spike
    f = fresh(ctx, D, "cosine", [(1, m2, np.arange(64, dtype=np.int64))], screen="int8", mid=mid, kernel="mfma")
    assert_same((ids, sc, _), f.search_vectors(None, 5, q))
    f.close()
    # the reverse: the block's only spike becomes Gaussian (s_blk must grow again for the rest of the block)
    g = (0.01 * rng.standard_normal(D)).astype(np.float32)
    found, changed = s.update_items([5], g[None])
    assert changed == 1
    m2[5] = g
    q2 = np.concatenate([m2[[3, 5, 17]], q[1:]])
    f = fresh(ctx, D, "cosine", [(1, m2, np.arange(64, dtype=np.int64))], screen="int8", mid=mid, kernel="mfma")
    got = s.search_vectors(None, 10, q2)
    assert_same(got, f.search_vectors(None, 10, q2))
    opos, _, _ = oracle.topk(q2, m2, 10)
    np.testing.assert_array_equal(got[0], opos)
    assert list(got[0][:3, 0]) == [3, 5, 17]
    s.close()
    f.close()


@pytest.mark.parametrize("quant", ["block", "rows"])
def test_mid_copy_on(ctx, oracle, quant):
    # block: the mid copy is built behind the int8 copy, with its block scales (updates re-pack whole blocks); rows: it was built
    # before the int8 copy existed, each row with its own scale (updates re-pack rows), and the int8 screen reads it since
    rng = np.random.default_rng(8)
    N, D = 20_000, 384
    m = new_vectors(rng, N, D)
    ids_col = rng.permutation(10 * N)[:N].astype(np.int64)
    q = rng.standard_normal((64, D)).astype(np.float32)
    upd_at = rng.choice(N, 1500, replace=False)
    vecs = new_vectors(rng, upd_at.size, D, (0.5, 4.0))
    m2 = m.copy()
    m2[upd_at] = vecs
    for metric in ("cosine", "dot"):
        parts = [(1, m[:12_000], ids_col[:12_000]), (2, m[12_000:], ids_col[12_000:])]
        s = fresh(ctx, D, metric, parts, screen="int8" if quant == "block" else "off", mid="on")
        if quant == "rows":
            s.set_screening_copy("int8")
            s.finalize()
        found, changed = s.update_items(ids_col[upd_at], vecs)
        assert found.all() and changed == upd_at.size
        f = fresh(ctx, D, metric, [(1, m2[:12_000], ids_col[:12_000]), (2, m2[12_000:], ids_col[12_000:])], screen="int8", mid="on")
        for kernel in ("wave", "mfma"):
            s.set_kernel(kernel)
            f.set_kernel(kernel)
            for B, k in ((4, 10), (64, 10), (8, 300)):  # 300: three passes below each other's ceilings
                got = s.search_vectors(None, k, q[:B])
                assert_same(got, f.search_vectors(None, k, q[:B]))
                if kernel == "mfma":
                    assert s.last_stats()["mid_copy"] == 1
                opos, _, ocnt = oracle.topk(q[:B], m2, k, METRIC[metric])
                np.testing.assert_array_equal(got[0], ids_col[opos])
                np.testing.assert_array_equal(got[2], ocnt)
            got = s.search_vectors([2], 10, q)  # a source filter
            assert_same(got, f.search_vectors([2], 10, q))
        s.close()
        f.close()


def plant_near_kth(rng, q, m, k, n_per_query):
    """Rows whose dot product with a query lands within 1e-3 of that query's k-th best dot over m (both sides)."""
    kth = np.sort(q.astype(np.float64) @ m.T.astype(np.float64), axis=1)[:, -k]
    out = []
    for b in range(q.shape[0]):
        qn = q[b] / np.linalg.norm(q[b])
        for j in range(n_per_query):
            noise = rng.standard_normal(q.shape[1])
            noise -= (noise @ qn) * qn
            t = kth[b] * (1.0 + (j - n_per_query / 2) * 2e-4) / np.linalg.norm(q[b])
            out.append((t * qn + 0.5 * noise).astype(np.float32))
    return np.stack(out)


def test_dot_norm_growth_int8(ctx, oracle):
    rng = np.random.default_rng(4)
    N, D, B, k = 20_000, 384, 16, 10
    m = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((B, D)).astype(np.float32)
    big = (4.0 * rng.standard_normal((100, D))).astype(np.float32)  # 4x the corpus's largest norm
    m1 = m.copy()
    big_at = rng.choice(N, 100, replace=False)
    m1[big_at] = big
    planted = plant_near_kth(rng, q, m1, k, 6)
    rest = np.setdiff1d(np.arange(N), big_at)
    plant_at = rng.choice(rest, planted.shape[0], replace=False)
    m2 = m1.copy()
    m2[plant_at] = planted
    at = np.concatenate([big_at, plant_at])
    s = fresh(ctx, D, "dot", [(1, m, np.arange(N, dtype=np.int64))], screen="int8", kernel="mfma")
    s.search_vectors(None, k, q)
    found, changed = s.update_items(at, m2[at])
    assert found.all() and changed == at.size
    f = fresh(ctx, D, "dot", [(1, m2, np.arange(N, dtype=np.int64))], screen="int8", kernel="mfma")
    for kk in (k, 200):
        got = s.search_vectors(None, kk, q)
        assert s.last_stats()["screening_copy"] == 2
        opos, _, ocnt = oracle.topk(q, m2, kk, 1)
        np.testing.assert_array_equal(got[0], opos)
        np.testing.assert_array_equal(got[2], ocnt)
        assert_same(got, f.search_vectors(None, kk, q))
    s.close()
    f.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_invalid_and_valid_rows(ctx, oracle, metric):
    rng = np.random.default_rng(9)
    N, D = 3000, 128
    m = rng.standard_normal((N, D)).astype(np.float32)
    m[77] = 0.0  # never searchable until it gets a vector
    q = np.concatenate([m[[10, 20]], rng.standard_normal((6, D)).astype(np.float32)])
    s = fresh(ctx, D, metric, [(1, m, np.arange(N, dtype=np.int64))], screen="int8")
    v = (3.0 * q[2]).astype(np.float32)
    nan = np.full(D, np.nan, np.float32)
    found, changed = s.update_items([10, 20, 77], np.stack([np.zeros(D, np.float32), nan, v]))
    assert found.all() and changed == 3
    m2 = m.copy()
    m2[10], m2[20], m2[77] = 0.0, np.nan, v
    f = fresh(ctx, D, metric, [(1, m2, np.arange(N, dtype=np.int64))], screen="int8")
    for kernel in ("wave", "mfma"):
        s.set_kernel(kernel)
        f.set_kernel(kernel)
        got = s.search_vectors(None, 50, q)
        assert_same(got, f.search_vectors(None, 50, q))
        assert not np.isin(got[0], [10, 20]).any()
        assert got[0][2, 0] == 77
        m3 = m2.copy()
        m3[20] = 0.0  # (the oracle's view of the NaN row: a zero row, never among these hits under either metric)
        opos, _, _ = oracle.topk(q, m3, 50, METRIC[metric])
        np.testing.assert_array_equal(got[0], opos)
    s.close()
    f.close()


def test_hidden_ids(ctx, oracle):
    rng = np.random.default_rng(6)
    N, D = 5000, 128
    m = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((4, D)).astype(np.float32)
    s = fresh(ctx, D, "cosine", [(1, m, np.arange(N, dtype=np.int64))], screen="int8", mid="on")
    assert s.hide_items([42, 43]) == 2
    found, changed = s.update_items([42, 1000], q[:2])
    assert found.all() and changed == 2
    assert s.hidden_rows == 2
    ids, sc, _ = s.search_vectors(None, 10, q)
    assert not np.isin(ids, [42, 43]).any() and ids[1, 0] == 1000
    assert s.unhide_items([42, 43]) == 2
    ids, sc, cnt = s.search_vectors(None, 10, q)
    assert ids[0, 0] == 42 and abs(sc[0, 0] - 1.0) <= 1e-7
    m2 = m.copy()
    m2[42], m2[1000] = q[0], q[1]
    f = fresh(ctx, D, "cosine", [(1, m2, np.arange(N, dtype=np.int64))], screen="int8", mid="on")
    assert_same((ids, sc, cnt), f.search_vectors(None, 10, q))
    s.close()
    f.close()


def test_ids_in_several_rows_and_sources_and_upsert(ctx, oracle):
    rng = np.random.default_rng(7)
    D = 64
    m = rng.standard_normal((400, D)).astype(np.float32)
    q = rng.standard_normal((3, D)).astype(np.float32)
    ids1 = np.arange(200, dtype=np.int64)
    ids2 = np.arange(200, 400, dtype=np.int64)
    ids2[5] = 7  # id 7: row 7 of source 1 and row 205 of source 2
    s = fresh(ctx, D, "cosine", [(1, m[:200], ids1), (2, m[200:], ids2)])
    before = s.search_vectors(None, 10, q)
    found, changed = s.update_items([123456, -5], rng.standard_normal((2, D)).astype(np.float32))
    assert not found.any() and changed == 0
    assert_same(s.search_vectors(None, 10, q), before)
    found, changed = s.update_items([7, 999999], np.stack([q[0], q[1]]))
    assert list(found) == [True, False] and changed == 2
    ids, sc, cnt = s.search_vectors(None, 2, q[:1])
    assert list(ids[0]) == [7, 7] and (np.abs(sc[0] - 1.0) <= 1e-7).all()
    m2 = m.copy()
    m2[7] = m2[205] = q[0]
    opos, _, _ = oracle.topk(q, m2, 10)
    np.testing.assert_array_equal(s.search_vectors(None, 10, q)[0], np.concatenate([ids1, ids2])[opos])
    s.close()
    # upsert: known ids are replaced, unknown ones appended to the source
    s = fresh(ctx, D, "cosine", [(1, m[:300], np.arange(1000, 1300, dtype=np.int64))])
    up_ids = np.array([1010, 5000, 1299, 5001], np.int64)
    up_rows = rng.standard_normal((4, D)).astype(np.float32)
    assert s.upsert_items(1, up_ids, up_rows) == (2, 2)
    assert s.num_rows == 302
    m3 = np.concatenate([m[:300], up_rows[[1, 3]]])
    m3[10], m3[299] = up_rows[0], up_rows[2]
    all_ids = np.concatenate([np.arange(1000, 1300), [5000, 5001]])
    q3 = np.concatenate([q, up_rows])
    ids, _, cnt = s.search_vectors(None, 10, q3)
    opos, _, ocnt = oracle.topk(q3, m3, 10)
    np.testing.assert_array_equal(ids, all_ids[opos])
    np.testing.assert_array_equal(cnt, ocnt)
    s.close()
    # implicit ids of synthetic rows: id0 + row
    s = pa.Searcher(ctx, 384, "cosine")
    s.add_synthetic(1, 5000, 0x51, first_row=100)
    s.finalize()
    ref = oracle.synth_rows(0x51, 100, 5000, 384)
    v = rng.standard_normal((4, 384)).astype(np.float32)
    found, changed = s.update_items([117, 4100, 99, 5100], v)  # 99 and 5100 lie outside the segment
    assert list(found) == [True, True, False, False] and changed == 2
    ref[17], ref[4000] = v[0], v[1]
    ids, _, _ = s.search_vectors(None, 5, v)
    opos, _, _ = oracle.topk(v, ref, 5)
    np.testing.assert_array_equal(ids, opos + 100)
    s.close()


def test_refusals(ctx):
    rng = np.random.default_rng(11)
    D = 64
    m = rng.standard_normal((500, D)).astype(np.float32)
    q = rng.standard_normal((4, D)).astype(np.float32)
    s = fresh(ctx, D, "cosine", [(1, m, np.arange(500, dtype=np.int64))])
    before = s.search_vectors(None, 10, q)
    v = rng.standard_normal((2, D)).astype(np.float32)
    with pytest.raises(_ffi.PcvError) as e:
        s.update_items([3, 3], v)  # duplicate ids
    assert e.value.status == PCV_ERR_INVALID
    assert_same(s.search_vectors(None, 10, q), before)
    s.add_rows(1, m[:1], np.array([900], np.int64))  # pending rows
    with pytest.raises(_ffi.PcvError) as e:
        s.update_items([3, 4], v)
    assert e.value.status == PCV_ERR_INVALID
    s.finalize()
    before = s.search_vectors(None, 10, q)
    out = ctx.alloc(4 * 10 * 24 + 64)
    s.search_device_begin(None, 10, q, out)  # a queued pass
    with pytest.raises(_ffi.PcvError) as e:
        s.update_items([3, 4], v)
    assert e.value.status == PCV_ERR_INVALID
    s.search_device_end()
    ctx.free(out)
    assert_same(s.search_vectors(None, 10, q), before)
    found, changed = s.update_items(np.zeros(0, np.int64), np.zeros((0, D), np.float32))  # n == 0: nothing
    assert found.size == 0 and changed == 0
    s.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_replayed_pass_sees_the_update(ctx, oracle, metric):
    rng = np.random.default_rng(3)
    m = rng.standard_normal((5000, 384)).astype(np.float32)
    q = rng.standard_normal((16, 384)).astype(np.float32)
    s = fresh(ctx, 384, metric, [(1, m, None)], screen="int8")
    for _ in range(3):  # the same pass shape again and again: captured as a graph and replayed
        first = s.search_vectors(None, 10, q)
    at = np.unique(np.concatenate([first[0][:, 0], rng.choice(5000, 40, replace=False)]))
    vecs = new_vectors(rng, at.size, 384, (2.0, 5.0) if metric == "dot" else (0.5, 2.0))  # dot: the largest norm grows
    s.update_items(at, vecs)
    m2 = m.copy()
    m2[at] = vecs
    ids, sc, cnt = s.search_vectors(None, 10, q)
    opos, _, ocnt = oracle.topk(q, m2, 10, METRIC[metric])
    np.testing.assert_array_equal(ids, opos)
    np.testing.assert_array_equal(cnt, ocnt)
    f = fresh(ctx, 384, metric, [(1, m2, None)], screen="int8")
    assert_same((ids, sc, cnt), f.search_vectors(None, 10, q))
    s.close()
    f.close()


def test_background_mid_build(ctx, oracle):
    rng = np.random.default_rng(31)
    n, d, k, B = 240_000, 128, 10, 64
    rows = oracle.synth_rows_clustered(0xC1, 0, n, d, 16, 0.004)
    probe = rows[rng.integers(0, n, B)]
    q = (probe + 0.002 * rng.standard_normal(probe.shape)).astype(np.float32)
    s = pa.Searcher(ctx, d, "cosine")
    s.add_rows(1, rows, np.arange(n, dtype=np.int64))
    s.finalize()
    s.set_mid_copy("auto")
    for _ in range(3):  # two passes above the trigger: the third call queues the build beside the searches
        s.search_vectors(None, k, q)
    top, _, _ = oracle.topk(q, rows, 3)
    at = np.unique(np.concatenate([top.reshape(-1), rng.choice(n, 2000, replace=False)]))
    vecs = rows[rng.integers(0, n, at.size)] + 0.002 * rng.standard_normal((at.size, d)).astype(np.float32)
    found, changed = s.update_items(at, vecs)  # at once: the build is settled first
    assert found.all() and changed == at.size
    m2 = rows.copy()
    m2[at] = vecs
    opos, _, ocnt = oracle.topk(q, m2, k)
    ids, _, cnt = s.search_vectors(None, k, q)
    np.testing.assert_array_equal(ids, opos)
    s.wait_background()
    ids, _, cnt = s.search_vectors(None, k, q)
    np.testing.assert_array_equal(ids, opos)
    np.testing.assert_array_equal(cnt, ocnt)
    assert s.last_stats()["mid_copy"] == 1
    s.close()


def _verify_topk(searcher, oracle, q, ids, pos, sc, k, n_total, rng, sample=256):
    """Size-independent checks of one result (as test_fullsize_gpu.py checks its results): scores re-derived by the oracle from
    the rows read back at the hits' positions `pos`, list sorted, and a random sample of other rows never beats the k-th score
    unless it is in the list."""
    rows, rid = searcher.get_rows(pos.reshape(-1))
    np.testing.assert_array_equal(rid, ids.reshape(-1))
    samp = rng.integers(0, n_total, sample)
    srows, sids = searcher.get_rows(samp)
    for b in range(q.shape[0]):
        ref = np.array([oracle.canonical_score(q[b], rows[b * k + j]) for j in range(k)])
        np.testing.assert_allclose(sc[b], ref.astype(np.float32), atol=1e-7)
        assert (np.diff(ref) <= 0).all()
        others = np.array([oracle.canonical_score(q[b], r) for r in srows])
        assert set(sids[others > ref[-1]]) <= set(ids[b])


def test_at_size(ctx, oracle):
    # 10M synthetic rows (implicit ids 0..) + a 2M explicit-id source fed in four adds (several segments); 100 000 ids updated
    # across both, 1 000 of them planted as the queries themselves
    N1, N2, D, k, SEED, ID2 = 10_000_000, 2_000_000, 384, 10, 0x5E7, 20_000_000
    rng = np.random.default_rng(12)
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, N1, SEED)
    for c in range(4):
        part = rng.standard_normal((N2 // 4, D), dtype=np.float32)
        s.add_rows(2, part, ID2 + c * (N2 // 4) + np.arange(N2 // 4, dtype=np.int64))
    s.finalize()
    assert s.num_segments >= 3 and s.num_rows == N1 + N2
    ids = np.concatenate([rng.choice(N1, 50_000, replace=False), ID2 + rng.choice(N2, 50_000, replace=False)]).astype(np.int64)
    vecs = rng.standard_normal((ids.size, D), dtype=np.float32)
    planted = rng.choice(ids.size, 1000, replace=False)
    q = vecs[planted].copy()
    found, changed = s.update_items(ids, vecs)
    assert found.all() and changed == ids.size
    assert s.num_rows == N1 + N2

    def pos_of(x):
        return np.where(x < N1, x, N1 + (x - ID2))

    samp = rng.choice(ids.size, 2000, replace=False)
    back, bid = s.get_rows(pos_of(ids[samp]))
    np.testing.assert_array_equal(bid, ids[samp])
    np.testing.assert_array_equal(back, vecs[samp])
    res_ids, sc, cnt = s.search_vectors(None, k, q)
    assert (cnt == k).all()
    np.testing.assert_array_equal(res_ids[:, 0], ids[planted])
    assert (np.abs(sc[:, 0] - 1.0) <= 1e-6).all()
    sub = rng.choice(1000, 16, replace=False)
    _verify_topk(s, oracle, q[sub], res_ids[sub], pos_of(res_ids[sub]), sc[sub], k, N1 + N2, rng)
    s.close()


def test_cpp_mirror_updates_on_gpu():
    src = os.path.join(ROOT, "tests", "cpp", "update_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "update_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "update_mirror_test: ok" in r.stdout
