"""The 6-bit screening copy (csrc/scan.h): AUTO builds it beside the int8 copy of large searchers, and 5..64-query
passes under the AUTO kernel choice screen it with an L2 bound before the int8 rows.  Forced here at small sizes
(PCV_SCAN_FLAGS bit 31) and compared with the oracle and with the same searcher made to keep to the int8 screen (bit 29)."""
import os

import numpy as np
import pytest

import perceive_amd as pa

pytestmark = pytest.mark.gpu

FORCE, FORBID = 1 << 31, 1 << 29


def build(ctx, corpus, metric="cosine", flags=FORCE, ids=None, mid="off"):
    s = pa.Searcher(ctx, corpus.shape[1], metric)
    s.set_tuning(flags)
    s.set_mid_copy(mid)  # (AUTO would drop the 6-bit copy for a mid copy on a crowded screen: test_six_gives_way_to_a_mid_copy)
    s.add_rows(1, corpus, ids)
    s.finalize()
    return s


def six_bytes(nblk, D):
    return nblk * (((D + 127) // 128 * 128) * 32 * 3 // 4 + 16)


@pytest.fixture(scope="module")
def g1000(golden_dir):
    return np.load(os.path.join(golden_dir, "scan_n1000_d384.npz"))


@pytest.mark.parametrize("B", [5, 33, 64])
def test_golden_1000_six(ctx, oracle, g1000, B):
    k = int(g1000["k"])
    s = build(ctx, g1000["corpus"])
    q = g1000["queries"][:B]
    ids, scores, counts = s.search_vectors(None, k, q)
    np.testing.assert_array_equal(ids, g1000["topk_f64"][:B])
    opos, osc, _ = oracle.topk(q, g1000["corpus"], k)
    np.testing.assert_array_equal(ids, opos)
    np.testing.assert_allclose(scores, osc.astype(np.float32), rtol=0, atol=1e-7)
    st = s.last_stats()
    assert st["screening_copy"] == 2 and st["screen_bits"] == 6 and st["scan_launches"] == 1
    assert st["bytes_streamed"] == six_bytes((1000 + 31) // 32, 384)
    assert st["narrow_survivors"] >= st["coarse_survivors"]
    # the int8 pin and the forbid bit keep the whole-int8 scan
    s.set_kernel("mfma")
    ids2, scores2, _ = s.search_vectors(None, k, q)
    assert s.last_stats()["screen_bits"] == 8
    np.testing.assert_array_equal(ids2, ids)
    np.testing.assert_array_equal(scores2, scores)
    s.set_kernel("auto")
    s.set_tuning(FORCE | FORBID)
    s.search_vectors(None, k, q)
    assert s.last_stats()["screen_bits"] == 8
    s.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_six_screen_on_rows_that_quantise_badly(ctx, oracle, metric):
    D = 384
    rng = np.random.default_rng(7 + len(metric))
    n = 4000
    heavy = rng.standard_cauchy((n, D)).astype(np.float32)
    onehot = np.zeros((500, D), np.float32)
    onehot[np.arange(500), rng.integers(0, D, 500)] = rng.standard_normal(500).astype(np.float32)
    q0 = rng.standard_normal(D).astype(np.float32)
    near = (q0[None, :] * (1.0 + 1e-4 * rng.standard_normal((3000, 1))) + 2e-4 * rng.standard_normal((3000, D))).astype(np.float32)
    gauss = rng.standard_normal((n, D)).astype(np.float32)
    corpus = np.concatenate([heavy, onehot, near, gauss])
    if metric == "cosine":
        corpus *= (10.0 ** rng.uniform(-15, 15, (corpus.shape[0], 1))).astype(np.float32)
    else:
        corpus *= (10.0 ** rng.uniform(-1.5, 1.5, (corpus.shape[0], 1))).astype(np.float32)
    corpus = corpus[rng.permutation(corpus.shape[0])]
    queries = np.concatenate([q0[None, :], rng.standard_normal((20, D)).astype(np.float32), rng.standard_cauchy((6, D)).astype(np.float32),
                              np.eye(D, dtype=np.float32)[:2], np.zeros((1, D), np.float32), corpus[:34]])
    s = build(ctx, corpus, metric=metric)
    for qs in (queries[:8], queries):
        ids, scores, _ = s.search_vectors(None, 10, qs)
        assert s.last_stats()["screen_bits"] == 6
        opos, osc, _ = oracle.topk(qs, corpus, 10, metric=1 if metric == "dot" else 0)
        np.testing.assert_array_equal(ids, opos)
    s.close()


def test_six_screen_with_hide_update_and_views(ctx, oracle):
    D, n = 384, 20_000
    rng = np.random.default_rng(3)
    corpus = rng.standard_normal((n, D)).astype(np.float32)
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    q = rng.standard_normal((40, D)).astype(np.float32)
    q[:8] = corpus[100:108]  # queries whose best rows get hidden, updated, shown again
    s = build(ctx, corpus, ids=ids)
    ref = build(ctx, corpus, ids=ids, flags=FORBID)

    def same(a, b, qs):
        ra = a.search_vectors(None, 10, qs)
        assert a.last_stats()["screen_bits"] == 6
        rb = b.search_vectors(None, 10, qs)
        assert b.last_stats()["screen_bits"] == 8
        for x, y in zip(ra, rb):
            np.testing.assert_array_equal(x, y)
        return ra

    same(s, ref, q)
    hid = ids[96:112]
    for t in (s, ref):
        t.hide_items(hid)
    r = same(s, ref, q)
    assert not np.isin(r[0], np.arange(96, 112)).any()
    big = (corpus[200:216] * 1e4).astype(np.float32)  # a larger norm: the block scales of their int8 blocks change
    for t in (s, ref):
        t.update_items(ids[200:216], big)
        t.unhide_items(hid)
    same(s, ref, q)
    allow = ids[rng.permutation(n)[:9000]]
    v, vr = s.view(allow), ref.view(allow)
    same(v, vr, q)
    v.close()
    vr.close()
    s.close()
    ref.close()


def test_six_gives_way_to_a_mid_copy(ctx, oracle):
    # every row within a quantisation step of the queries: the coarse screen lets thousands through, AUTO builds the mid copy
    # after two such passes and frees the 6-bit copy before it does; the results stay the oracle's
    D = 384
    rng = np.random.default_rng(5)
    q0 = rng.standard_normal(D).astype(np.float32)
    corpus = (q0[None, :] + 1e-3 * rng.standard_normal((30_000, D))).astype(np.float32)
    q = (q0[None, :] + 1e-3 * rng.standard_normal((16, D))).astype(np.float32)
    s = build(ctx, corpus, mid="auto")
    bits = []
    for _ in range(4):
        ids, _, _ = s.search_vectors(None, 10, q)
        bits.append(s.last_stats()["screen_bits"])
        np.testing.assert_array_equal(ids, oracle.topk(q, corpus, 10)[0])
    s.wait_background()
    ids, _, _ = s.search_vectors(None, 10, q)
    np.testing.assert_array_equal(ids, oracle.topk(q, corpus, 10)[0])
    assert bits[0] == 6 and s.last_stats()["screen_bits"] == 8
    s.close()
