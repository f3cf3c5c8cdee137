"""GPU: hidden items (pcv_searcher_hide_ids).  The reference result is always the oracle over the rows with the hidden ones
REMOVED, positions mapped back (removal keeps the order, so ties agree); unhiding restores every result bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SCREEN_KIND = {"int8": 2, "bf16": 1, "off": 0}


@pytest.fixture(scope="module")
def g1000(golden_dir):
    return np.load(os.path.join(golden_dir, "scan_n1000_d384.npz"))


def oracle_without(oracle, q, rows, hidden_pos, k, metric="cosine"):
    """oracle.topk over the rows not in hidden_pos -> (positions in `rows`, f64 scores, counts)"""
    keep = np.setdiff1d(np.arange(rows.shape[0]), np.asarray(hidden_pos, np.int64))
    pos, sc, cnt = oracle.topk(q, rows[keep], k, metric={"cosine": 0, "dot": 1}[metric])
    return np.where(pos >= 0, keep[np.maximum(pos, 0)], -1), sc, cnt


def queries_256(g1000):
    rng = np.random.default_rng(256)
    return np.concatenate([g1000["queries"], rng.standard_normal((192, 384)).astype(np.float32)])


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("B", [1, 4, 64, 256])
@pytest.mark.parametrize("kernel", ["auto", "wave", "mfma"])
@pytest.mark.parametrize("screen", ["int8", "bf16", "off"])
def test_golden_with_hidden_rows(ctx, oracle, g1000, screen, kernel, B, metric):
    corpus, k = g1000["corpus"], 10
    q = queries_256(g1000)[:B]
    s = pa.Searcher(ctx, 384, metric)
    s.set_screening_copy(screen)
    s.add_rows(1, corpus)  # ids = positions
    s.finalize()
    s.set_kernel(kernel)
    top, _, _ = s.search_vectors(None, 3, q)
    rng = np.random.default_rng(B)
    hidden = np.unique(np.concatenate([top.reshape(-1), rng.choice(1000, 50, replace=False)]))
    assert s.hide_items(hidden) == hidden.size
    np.testing.assert_array_equal(s.hidden_items(), hidden)
    assert s.hidden_rows == hidden.size and s.num_rows == 1000
    ids, sc, cnt = s.search_vectors(None, k, q)
    opos, osc, ocnt = oracle_without(oracle, q, corpus, hidden, k, metric)
    np.testing.assert_array_equal(ids, opos)
    np.testing.assert_array_equal(cnt, ocnt)
    assert (cnt == k).all() and not np.isin(ids, hidden).any()
    if metric == "cosine":
        np.testing.assert_allclose(sc, osc.astype(np.float32), rtol=0, atol=1e-7)
    st = s.last_stats()
    mfma = kernel == "mfma" or (kernel == "auto" and (B > 4 or screen != "off"))
    assert st["kernel_used"] == (2 if mfma else 1)
    assert st["screening_copy"] == (SCREEN_KIND[screen] if mfma else 0)
    s.close()


@pytest.mark.parametrize("mid", ["off", "on"])
@pytest.mark.parametrize("screen", ["int8", "bf16", "off"])
def test_unhide_restores_bit_identically(ctx, oracle, screen, mid):
    rng = np.random.default_rng(7)
    N, D = 20_000, 384
    m = (rng.standard_normal((N, D)) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
    ids_col = rng.permutation(10 * N)[:N].astype(np.int64)
    q = rng.standard_normal((64, D)).astype(np.float32)
    for metric in ("cosine", "dot"):
        s = pa.Searcher(ctx, D, metric)
        s.set_screening_copy(screen)
        s.set_mid_copy(mid)
        s.add_rows(1, m[:12_000], ids_col[:12_000])
        s.add_rows(2, m[12_000:], ids_col[12_000:])
        s.finalize()
        before = {}
        for kernel in ("wave", "mfma"):
            s.set_kernel(kernel)
            for B, k in ((4, 10), (64, 10), (8, 300)):  # 300: three passes below each other's ceilings
                before[kernel, B, k] = s.search_vectors(None, k, q[:B])
        top = before["mfma", 64, 10][0][:, :5].reshape(-1)
        hide = np.unique(np.concatenate([top, rng.choice(ids_col, 2000, replace=False)]))
        assert s.hide_items(hide) == hide.size
        ids, _, cnt = s.search_vectors(None, 10, q)
        assert (cnt == 10).all() and not np.isin(ids, hide).any()
        assert s.unhide_items(hide) == hide.size
        assert s.hidden_items().size == 0 and s.hidden_rows == 0
        for (kernel, B, k), (ids0, sc0, cnt0) in before.items():
            s.set_kernel(kernel)
            ids1, sc1, cnt1 = s.search_vectors(None, k, q[:B])
            np.testing.assert_array_equal(ids1, ids0)
            np.testing.assert_array_equal(sc1.view(np.uint32), sc0.view(np.uint32))
            np.testing.assert_array_equal(cnt1, cnt0)
        s.close()


def test_replayed_pass_sees_hidden_rows(ctx, oracle):
    rng = np.random.default_rng(3)
    m = rng.standard_normal((5000, 384)).astype(np.float32)
    q = rng.standard_normal((16, 384)).astype(np.float32)
    s = pa.Searcher(ctx, 384, "cosine")
    s.add_rows(1, m)
    s.finalize()
    first = s.search_vectors(None, 10, q)
    second = s.search_vectors(None, 10, q)  # the same pass shape again: captured as a graph and replayed from now on
    np.testing.assert_array_equal(first[0], second[0])
    hit = int(first[0][0, 0])
    assert s.hide_items([hit]) == 1
    ids, sc, _ = s.search_vectors(None, 10, q)
    assert hit not in ids
    opos, osc, _ = oracle_without(oracle, q, m, [hit], 10)
    np.testing.assert_array_equal(ids, opos)
    assert s.unhide_items([hit]) == 1
    ids, sc, _ = s.search_vectors(None, 10, q)
    np.testing.assert_array_equal(ids, first[0])
    np.testing.assert_array_equal(sc, first[1])
    s.close()


@pytest.mark.parametrize("mid", ["off", "on"])
def test_unhide_repacks_the_block(ctx, mid):
    # Row 35 dominates its 32-row block of the int8 copy (one component at 0.9).  Hidden, the block is re-packed by a finalize
    # that appends rows 40..49 into it: s_blk is then taken without row 35, far above 127 / its max.  Unhidden, its int8 values
    # must not clip: it is the top hit of a query equal to it, ahead of its near copies.
    rng = np.random.default_rng(35)
    D = 384
    m = (0.01 * rng.standard_normal((50, D))).astype(np.float32)
    m[35, 0] = 0.9
    m[:6] = m[35] + 0.005 * rng.standard_normal((6, D)).astype(np.float32)  # block 0: near copies (cos ~0.99) raise the threshold
    s = pa.Searcher(ctx, D, "cosine")
    s.set_screening_copy("int8")
    s.set_mid_copy(mid)
    s.set_kernel("mfma")
    s.add_rows(1, m[:40], np.arange(40, dtype=np.int64))
    s.finalize()
    assert s.hide_items([35]) == 1
    s.add_rows(1, m[40:], np.arange(40, 50, dtype=np.int64))
    s.finalize()
    assert s.num_segments == 1 and s.num_rows == 50
    q = np.concatenate([m[35:36], rng.standard_normal((7, D)).astype(np.float32)])
    ids, sc, _ = s.search_vectors(None, 5, q)
    assert 35 not in ids
    assert s.unhide_items([35]) == 1
    ids, sc, _ = s.search_vectors(None, 5, q)
    st = s.last_stats()
    assert st["kernel_used"] == 2 and st["screening_copy"] == 2 and st["mid_copy"] == (1 if mid == "on" else 0)
    assert ids[0, 0] == 35 and set(ids[0, 1:]) <= set(range(6))
    assert abs(sc[0, 0] - 1.0) < 1e-7
    s.close()


def test_the_set_persists(ctx, oracle):
    rng = np.random.default_rng(5)
    m = rng.standard_normal((300, 128)).astype(np.float32)
    q = m[[10, 250]] + 0.01 * rng.standard_normal((2, 128)).astype(np.float32)
    s = pa.Searcher(ctx, 128, "cosine")
    s.add_rows(1, m[:200], np.arange(1000, 1200, dtype=np.int64))
    s.finalize()
    assert s.hide_items([1250, 1010, 99999]) == 1  # 1250 and 99999: no row has them yet
    np.testing.assert_array_equal(s.hidden_items(), [1010, 1250, 99999])
    s.add_rows(1, m[200:], np.arange(1200, 1300, dtype=np.int64))
    s.finalize()
    assert s.hidden_rows == 2
    ids, _, _ = s.search_vectors(None, 20, q)
    assert not np.isin(ids, [1010, 1250]).any()
    opos, _, _ = oracle_without(oracle, q, m, [10, 250], 20)
    np.testing.assert_array_equal(ids, opos + 1000)
    # rebuild_source: the staged replacement rows honour the set, and the set is not forgotten
    rows = [(1000 + i, 1, m[i]) for i in range(300)]
    s.rebuild_source(rows, 1)
    assert s.num_rows == 300 and s.hidden_rows == 2
    np.testing.assert_array_equal(s.hidden_items(), [1010, 1250, 99999])
    ids2, _, _ = s.search_vectors(None, 20, q)
    np.testing.assert_array_equal(ids2, ids)
    pa._ffi.check(pa._ffi.lib().pcv_searcher_clear_source(s._handle, 1))
    s.finalize()
    np.testing.assert_array_equal(s.hidden_items(), [1010, 1250, 99999])
    assert s.hidden_rows == 0
    s.close()


def test_edge_cases(ctx, oracle):
    rng = np.random.default_rng(6)
    m = rng.standard_normal((400, 64)).astype(np.float32)
    q = rng.standard_normal((3, 64)).astype(np.float32)
    s = pa.Searcher(ctx, 64, "cosine")
    s.add_rows(1, m[:150], np.arange(150, dtype=np.int64))
    s.add_rows(2, m[150:], np.arange(150, 400, dtype=np.int64))
    s.finalize()
    for kernel in ("wave", "mfma"):
        s.set_kernel(kernel)
        s.hide_items(np.arange(150))  # every row of source 1
        assert s.search_vectors([1], 10, q)[2].sum() == 0
        ids, _, cnt = s.search_vectors(None, 10, q)
        assert (cnt == 10).all() and (ids >= 150).all()
        s.hide_items(np.arange(150, 397))  # all but 3 rows
        ids, _, cnt = s.search_vectors(None, 10, q)
        assert (cnt == 3).all() and (np.sort(ids[:, :3], axis=1) == [397, 398, 399]).all()
        assert s.unhide_items(np.arange(400)) == 397
    s.close()
    # the same id in two sources: both rows go
    s = pa.Searcher(ctx, 64, "cosine")
    s.add_rows(1, m[:2], np.array([7, 8], np.int64))
    s.add_rows(2, m[2:4], np.array([7, 9], np.int64))
    s.finalize()
    assert s.hide_items([7]) == 2
    ids, _, cnt = s.search_vectors(None, 4, q)
    assert (cnt == 2).all() and not (ids == 7).any()
    s.close()
    # implicit ids of synthetic rows: id0 + row
    s = pa.Searcher(ctx, 384, "cosine")
    s.add_synthetic(1, 5000, 0x51, first_row=100)
    s.finalize()
    ref = oracle.synth_rows(0x51, 100, 5000, 384)
    q2 = ref[[17, 4000]]
    ids, _, _ = s.search_vectors(None, 5, q2)
    assert list(ids[:, 0]) == [117, 4100]
    assert s.hide_items([117, 4100, 99, 5100]) == 2  # 99 and 5100 lie outside the segment
    ids, _, _ = s.search_vectors(None, 5, q2)
    opos, _, _ = oracle_without(oracle, q2, ref, [17, 4000], 5)
    np.testing.assert_array_equal(ids, opos + 100)
    s.close()


def test_clustered_mid_copy_top_rows_hidden(ctx, oracle):
    rng = np.random.default_rng(31)
    n, d, k, B = 120_000, 128, 10, 8
    rows = oracle.synth_rows_clustered(0xC1, 0, n, d, 16, 0.004)
    q = (rows[rng.integers(0, n, B)] + 0.002 * rng.standard_normal((B, d))).astype(np.float32)
    s = pa.Searcher(ctx, d, "cosine")
    s.set_mid_copy("on")
    s.add_rows(1, rows, np.arange(n, dtype=np.int64))
    s.finalize()
    top, _, _ = oracle.topk(q, rows, 200)
    hidden = np.unique(top.reshape(-1))
    assert s.hide_items(hidden) == hidden.size
    ids, sc, _ = s.search_vectors(None, k, q)
    st = s.last_stats()
    assert st["mid_copy"] == 1 and st["screening_copy"] == 2
    opos, osc, _ = oracle_without(oracle, q, rows, hidden, k)
    np.testing.assert_array_equal(ids, opos)
    np.testing.assert_allclose(sc, osc.astype(np.float32), rtol=0, atol=1e-7)
    s.close()


def test_sharded_with_a_hidden_boundary_row(ctx, oracle):
    n, D, k, SEED = 300_000, 384, 10, 0x5A
    q = oracle.synth_rows(SEED + 1, 0, 4, D)
    lo1, _ = pa.shard_bounds(n, 1, 3)
    ref = oracle.synth_rows(SEED, 0, n, D)
    top, _, _ = oracle.topk(q, ref, 3)
    hidden = np.unique(np.concatenate([top.reshape(-1), [lo1 - 1, lo1]]))
    whole = pa.Searcher(ctx, D, "cosine")
    whole.add_synthetic(1, n, SEED)
    whole.finalize()
    whole.hide_items(hidden)
    w_ids, w_sc, _ = whole.search_vectors(None, k, q)
    whole.close()
    opos, _, _ = oracle_without(oracle, q, ref, hidden, k)
    np.testing.assert_array_equal(w_ids, opos)
    lists = ctx.alloc(3 * 4 * k * 24)
    shards, changed = [], 0
    for r in range(3):
        lo, hi = pa.shard_bounds(n, r, 3)
        s = pa.Searcher(ctx, D, "cosine")
        s.add_synthetic(1, hi - lo, SEED, first_row=lo)
        s.finalize()
        s.set_shard_offset(lo)
        sh = pa.ShardedSearcher(None, "cosine", D, searcher=s, ctx=ctx, comm=type("C", (), {"world": 3, "rank": r})())
        changed += sh.hide_items(hidden)  # every rank the same ids
        s.search_device_begin(None, k, q, lists + r * 4 * k * 24)
        s.search_device_end()
        shards.append(s)
    assert changed == hidden.size
    m_ids, m_sc, _ = pa.merge_topk(ctx, "cosine", D, lists, 3, 4, k)
    np.testing.assert_array_equal(m_ids, w_ids)
    np.testing.assert_array_equal(m_sc, w_sc)
    ctx.free(lists)
    for s in shards:
        s.close()


def test_full_size_10m(ctx, oracle):
    import test_fullsize_gpu as fs

    N, D, B, k, SEED = 10_000_000, 384, 64, 10, 0x10B
    rng = np.random.default_rng(10)
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, N, SEED)
    s.finalize()
    q = oracle.synth_rows(SEED + 3, 0, B, D)
    ids0, sc0, cnt0 = s.search_vectors(None, k, q)
    hidden = np.unique(np.concatenate([ids0.reshape(-1), rng.integers(0, N, 100_000)]))
    assert s.hide_items(hidden) == hidden.size
    ids, sc, cnt = s.search_vectors(None, k, q)
    assert (cnt == k).all() and not np.isin(ids, hidden).any()
    fs._verify_topk(s, oracle, q, ids, sc, k, N, rng)
    assert s.unhide_items(hidden) == hidden.size
    ids1, sc1, cnt1 = s.search_vectors(None, k, q)
    np.testing.assert_array_equal(ids1, ids0)
    np.testing.assert_array_equal(sc1.view(np.uint32), sc0.view(np.uint32))
    np.testing.assert_array_equal(cnt1, cnt0)
    s.close()


def test_cpp_mirror_hides_on_gpu():
    src = os.path.join(ROOT, "tests", "cpp", "hide_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "hide_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hide_mirror_test: ok" in r.stdout
