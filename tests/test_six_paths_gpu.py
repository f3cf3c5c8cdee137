"""GPU: the 6-bit screen (csrc/scan.h) away from 384 features and small single segments — its one-, two- and
three-chunk forms against the oracle and against the int8 screen of the same rows, the shapes at which the pass must step back to
the int8 form, the screen's survivor counts against the float64 model of tests/six_ref.py, many segments, waves that stream several
blocks, blocks with nothing to search, a crowded screen, and the mutations of a finalized segment."""
import numpy as np
import pytest

import perceive_amd as pa
import six_ref
from test_six_gpu import FORBID, FORCE, build, six_bytes

pytestmark = pytest.mark.gpu

WIDTHS = [64, 100, 128, 136, 200, 256, 260, 384]  # chunks of 128 features: 1, 1, 1, 2, 2, 2, 3, 3
METRIC = {"cosine": 0, "dot": 1}


def want(oracle, queries, rows, k, metric, ids=None):
    """oracle.topk as a searcher reports it: (ids, f32 scores) with -1 / NaN behind a query's last hit; rows the oracle gives no
    score (zero rows under cosine, non-finite rows) are no hits"""
    opos, osc, _ = oracle.topk(queries, rows, k, metric=METRIC[metric])
    score = np.where(opos >= 0, six_ref.reported(osc, metric, rows.shape[1]), np.float32(np.nan)).astype(np.float32)
    return (opos if ids is None else np.where(opos >= 0, ids[np.maximum(opos, 0)], -1)), score


def same_hits(got, ref):
    for x, y in zip(got, ref):
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


def mixed_queries(rng, corpus, n):
    """Gaussian, stored, one-hot, all-zero and heavy-tailed queries, every kind among the first five"""
    D = corpus.shape[1]
    q = rng.standard_normal((n, D)).astype(np.float32)
    q[1::5] = corpus[rng.integers(0, corpus.shape[0], len(q[1::5]))]
    q[2::5] = np.eye(D, dtype=np.float32)[rng.integers(0, D, len(q[2::5]))]
    q[3] = 0.0
    q[4::5] = rng.standard_cauchy((len(q[4::5]), D)).astype(np.float32)
    return q


# ---- widths and tiles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("D", WIDTHS)
def test_every_width_and_tile(ctx, oracle, D, metric):
    n = 1007  # 31 full blocks and one of 15 rows
    rng = np.random.default_rng(40 + D)
    corpus = (rng.standard_normal((n, D)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    queries = mixed_queries(rng, corpus, 64)
    ref_ids, ref_sc = want(oracle, queries, corpus, 10, metric)
    s, t = build(ctx, corpus, metric=metric), build(ctx, corpus, metric=metric, flags=FORBID)
    for B in (5, 32, 33, 64):
        got = s.search_vectors(None, 10, queries[:B])
        st = s.last_stats()
        np.testing.assert_array_equal(got[0], ref_ids[:B])
        np.testing.assert_allclose(got[1], ref_sc[:B], rtol=0, atol=1e-7)
        assert st["screen_bits"] == 6 and st["scan_launches"] == 1
        assert st["bytes_streamed"] == six_bytes((n + 31) // 32, D)
        assert st["narrow_survivors"] >= st["coarse_survivors"]
        twin = t.search_vectors(None, 10, queries[:B])
        assert t.last_stats()["screen_bits"] == 8
        same_hits(got, twin)
    s.close()
    t.close()


# ---- where the pass must keep to the int8 form (mfma8_six_pass) -----------------------------------------------------------------------
@pytest.mark.parametrize("D,B,flags", [(128, 4, FORCE), (128, 65, FORCE), (388, 16, FORCE), (128, 16, FORCE | 1),
                                       (128, 16, FORCE | (3 << 24)), (128, 16, FORCE | (1 << 28))])
def test_steps_back_to_int8(ctx, oracle, D, B, flags):
    rng = np.random.default_rng(7 * D + B)
    corpus = rng.standard_normal((1007, D)).astype(np.float32)
    queries = mixed_queries(rng, corpus, B)
    s = build(ctx, corpus, flags=flags)
    got = s.search_vectors(None, 10, queries)
    st = s.last_stats()
    assert st["screening_copy"] == 2 and st["screen_bits"] == 8
    ref_ids, ref_sc = want(oracle, queries, corpus, 10, "cosine")
    np.testing.assert_array_equal(got[0], ref_ids)
    np.testing.assert_allclose(got[1], ref_sc, rtol=0, atol=1e-7)
    if D <= 384:  # the copy is there: the same searcher streams it at a shape the form takes
        s.set_tuning(FORCE)
        s.search_vectors(None, 10, mixed_queries(rng, corpus, 16))
        assert s.last_stats()["screen_bits"] == 6
    s.close()


# ---- fixed thresholds: the screen as numbers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("D", [100, 200, 384])
def test_survivor_counts_are_the_models(ctx, oracle, D, metric):
    """A range pass fixes its thresholds before the scan (range_thresholds_kernel; every row is of class 1 of its ceiling, so
    neither the seed nor the drain wave's offers raise one), so the rows its screens let through are a function of the copies and
    the query constants alone — and six_ref computes that function in float64.  narrow_survivors (rows past the 6-bit test) and
    coarse_survivors (of those, the rows past the int8 test) must lie between the model's counts with both tests tightened and
    loosened by six_ref.kernel_slack(D); test_six_bound.py::test_model_bracket_is_tight holds the two within 2 % of each other
    for these inputs.  A wrong r_blk, n_blk, A_q, E_q or Wn_q, or a bit unpacked to the wrong place, moves the counts by far more
    and leaves every result exact."""
    corpus, queries, bounds, in_range, opos, orep = six_ref.range_case(oracle, D, metric)
    rows = six_ref.Rows(corpus, metric)
    qs = six_ref.Queries(queries, rows)
    tau = six_ref.range_tau(bounds, queries, rows)
    slack = six_ref.kernel_slack(D)
    lo6, lo8 = (int(x.sum()) for x in six_ref.keeps(rows, qs, tau, -slack))
    hi6, hi8 = (int(x.sum()) for x in six_ref.keeps(rows, qs, tau, +slack))
    s, t = build(ctx, corpus, metric=metric), build(ctx, corpus, metric=metric, flags=FORBID)
    got = s.search_range(None, bounds, queries, 256)
    st = s.last_stats()
    twin = t.search_range(None, bounds, queries, 256)
    st8 = t.last_stats()
    print(f"D={D} {metric}: 6-bit survivors {st['narrow_survivors']} (model {lo6} .. {hi6}), of those past the int8 test "
          f"{st['coarse_survivors']} (model {lo8} .. {hi8}); int8 screen alone {st8['coarse_survivors']}")
    assert st["screen_bits"] == 6 and st["scan_launches"] == 1 and st8["screen_bits"] == 8 and st8["scan_launches"] == 1
    np.testing.assert_array_equal(got[2], in_range)
    assert not got[3].any()
    for q in range(64):
        m = int(in_range[q])
        np.testing.assert_array_equal(got[0][q, :m], opos[q, :m])
        np.testing.assert_allclose(got[1][q, :m], orep[q, :m], rtol=0, atol=1e-7)
        np.testing.assert_array_equal(twin[0][q, :m], got[0][q, :m])
        np.testing.assert_array_equal(twin[1][q, :m].view(np.uint32), got[1][q, :m].view(np.uint32))
    assert lo6 <= st["narrow_survivors"] <= hi6
    assert lo8 <= st["coarse_survivors"] <= hi8
    assert st["coarse_survivors"] <= st8["coarse_survivors"]
    s.close()
    t.close()


# ---- many segments --------------------------------------------------------------------------------------------------------------------
def test_forty_segments(ctx, oracle):
    D = 200
    rng = np.random.default_rng(11)
    sizes = [1, 31, 32, 33, 70, 129, 200, 95] * 5
    s = pa.Searcher(ctx, D, "cosine")
    s.set_tuning(FORCE)
    s.set_mid_copy("off")
    parts, part_ids = [], []
    for i, m in enumerate(sizes):
        rows = rng.standard_normal((m, D)).astype(np.float32)
        explicit = i % 3 != 1  # the other sources have implicit ids: the row's number in its source
        ids = (100_000 * (i + 1) + rng.permutation(10 * m)[:m]).astype(np.int64) if explicit else np.arange(m, dtype=np.int64)
        s.add_rows(i + 1, rows, ids if explicit else None)
        s.finalize()
        parts.append(rows)
        part_ids.append(ids)
    assert s.num_segments == 40 and s.num_rows == sum(sizes)
    queries = mixed_queries(rng, np.concatenate(parts), 64)

    def check(nblocks):
        corpus, ids = np.concatenate(parts), np.concatenate(part_ids)
        for B in (64, 8):
            got = s.search_vectors(None, 10, queries[:B])
            st = s.last_stats()
            ref_ids, ref_sc = want(oracle, queries[:B], corpus, 10, "cosine", ids)
            np.testing.assert_array_equal(got[0], ref_ids)
            np.testing.assert_allclose(got[1], ref_sc, rtol=0, atol=1e-7)
            assert st["screen_bits"] == 6 and st["scan_launches"] == 1
            assert st["bytes_streamed"] == sum(six_bytes(b, D) for b in nblocks)

    check([(m + 31) // 32 for m in sizes])
    # the last finalized segment grows through its unfinished block (95 rows: two blocks and 31 rows): its 6-bit copy grows with it
    more = rng.standard_normal((37, D)).astype(np.float32)
    more[5] = queries[0] * 3.0  # a new row that must be found
    more_ids = (5_000_000 + np.arange(37)).astype(np.int64)
    s.add_rows(40, more, more_ids)
    s.finalize()
    assert s.num_segments == 40 and s.num_rows == sum(sizes) + 37
    parts[-1], part_ids[-1] = np.concatenate([parts[-1], more]), np.concatenate([part_ids[-1], more_ids])
    check([(m + 31) // 32 for m in sizes[:-1]] + [(95 + 37 + 31) // 32])
    assert s.search_vectors(None, 10, queries[:8])[0][0, 0] == more_ids[5]
    s.close()


# ---- more than one block per wave ----------------------------------------------------------------------------------------------------
def compute_units():
    try:
        import torch

        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        return 256  # MI355X


@pytest.mark.parametrize("D,metric", [(128, "cosine"), (256, "dot")])
def test_waves_that_stream_several_blocks(ctx, oracle, D, metric):
    """One 12-wave workgroup per CU, eleven of its waves streaming: with more than 2 x 11 x CUs blocks some waves take a third
    block, each 11 x CUs blocks after the one before — across the boundaries of five segments of unequal size.  The reference is
    the oracle's canonical ranking of each query's 256 best rows by an f32 matrix product (the k-th best is far inside them)."""
    wave_stride = 11 * compute_units()
    n = (2 * wave_stride + 200) * 32 + 9
    rng = np.random.default_rng(D)
    corpus = rng.standard_normal((n, D), dtype=np.float32)
    cuts = [0, n // 11, n // 11 + 4097, n // 2 + 13, n - 70_001, n]
    queries = rng.standard_normal((64, D), dtype=np.float32)
    queries[1] = corpus[cuts[2] - 1]
    queries[2] = corpus[n - 1]
    s, t = (pa.Searcher(ctx, D, metric) for _ in range(2))
    for x, flags in ((s, FORCE), (t, FORBID)):
        x.set_tuning(flags)
        x.set_mid_copy("off")
        for i in range(5):
            x.add_rows(i + 1, corpus[cuts[i] : cuts[i + 1]])
        x.finalize()
        assert x.num_segments == 5
    ids = np.concatenate([np.arange(cuts[i + 1] - cuts[i], dtype=np.int64) for i in range(5)])  # implicit: the row's number in its source
    if metric == "cosine":
        approx = (queries / np.linalg.norm(queries, axis=1, keepdims=True)) @ (corpus / np.linalg.norm(corpus, axis=1, keepdims=True)).T
    else:
        approx = queries @ corpus.T
    ref_ids, ref_sc = np.empty((64, 10), np.int64), np.empty((64, 10), np.float32)
    for q in range(64):
        cand = np.sort(np.argpartition(-approx[q], 256)[:256])  # ascending: the oracle's ties go to the lower position
        assert np.sort(approx[q, cand])[0] < np.sort(approx[q, cand])[-10] - 1e-3 * np.abs(approx[q]).max()
        i, sc = want(oracle, queries[q : q + 1], corpus[cand], 10, metric, ids[cand])
        ref_ids[q], ref_sc[q] = i[0], sc[0]
    for B in (64, 8):
        got = s.search_vectors(None, 10, queries[:B])
        st = s.last_stats()
        assert st["screen_bits"] == 6 and st["scan_launches"] == 1
        assert st["bytes_streamed"] == sum(six_bytes((cuts[i + 1] - cuts[i] + 31) // 32, D) for i in range(5))
        np.testing.assert_array_equal(got[0], ref_ids[:B])
        np.testing.assert_allclose(got[1], ref_sc[:B], rtol=0, atol=1e-7)
        twin = t.search_vectors(None, 10, queries[:B])
        assert t.last_stats()["screen_bits"] == 8
        same_hits(got, twin)
    s.close()
    t.close()


# ---- blocks with nothing to search --------------------------------------------------------------------------------------------------
def test_blocks_without_a_searchable_row(ctx, oracle):
    D, n = 136, 32 * 12 + 5
    rng = np.random.default_rng(13)
    corpus = rng.standard_normal((n, D)).astype(np.float32)
    for b in (0, 5, 11):  # the first block, one in the middle, the last full one: scale8 = NaN
        corpus[32 * b : 32 * b + 32] = 0.0
    lone = corpus[32 * 7 + 17].copy()
    corpus[32 * 7 : 32 * 7 + 32] = 0.0
    corpus[32 * 7 + 17] = lone
    ids = (np.arange(n, dtype=np.int64) * 7 + 3)
    queries = mixed_queries(rng, corpus[32:64], 16)
    queries[0] = lone
    s = build(ctx, corpus, ids=ids)
    zero = np.flatnonzero(~corpus.any(axis=1))
    assert zero.size == 4 * 32 - 1

    def check(hidden):
        ref = corpus.copy()
        ref[hidden] = 0.0  # (no score under cosine: the oracle leaves them out and keeps the positions)
        for B in (16, 5):
            got = s.search_vectors(None, 10, queries[:B])
            assert s.last_stats()["screen_bits"] == 6
            ref_ids, ref_sc = want(oracle, queries[:B], ref, 10, "cosine", ids)
            np.testing.assert_array_equal(got[0], ref_ids)
            np.testing.assert_allclose(got[1], ref_sc, rtol=0, atol=1e-7)
            assert not np.isin(got[0], ids[zero]).any() and not np.isin(got[0], ids[hidden]).any()
        return got

    got = check(np.zeros(0, np.int64))
    assert got[0][0, 0] == ids[32 * 7 + 17]
    block3 = np.arange(96, 128)
    assert s.hide_items(ids[block3]) == 32
    check(block3)
    assert s.hide_items(ids[[32 * 7 + 17]]) == 1  # now block 7 has nothing either
    check(np.append(block3, 32 * 7 + 17))
    assert s.unhide_items(ids[np.append(block3, 32 * 7 + 17)]) == 33
    got = check(np.zeros(0, np.int64))
    assert got[0][0, 0] == ids[32 * 7 + 17]
    s.close()


# ---- a crowded screen at two chunks -------------------------------------------------------------------------------------------------
def test_crowded_screen_at_two_chunks(ctx, oracle):
    # every row within a quantisation step of the queries: the 6-bit screen lets all of them through, the survivor ring and the
    # drain wave's stack fill up; with the mid copy off the pass stays on the 6-bit copy
    D, n = 256, 20_000
    rng = np.random.default_rng(5)
    q0 = rng.standard_normal(D).astype(np.float32)
    corpus = (q0[None, :] + 1e-3 * rng.standard_normal((n, D))).astype(np.float32)
    queries = (q0[None, :] + 1e-3 * rng.standard_normal((64, D))).astype(np.float32)
    s = build(ctx, corpus)
    opos = oracle.topk(queries, corpus, 128)[0]  # (the best 10 are the first 10 of the best 128)
    for k in (10, 128):
        ids, _, counts = s.search_vectors(None, k, queries)
        st = s.last_stats()
        assert st["screen_bits"] == 6 and st["narrow_survivors"] >= n
        assert (counts == k).all()
        np.testing.assert_array_equal(ids, opos[:, :k])
    s.close()


# ---- the mutations of a finalized segment, away from 384 ------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [100, 200])
def test_mutations_keep_the_copy_current(ctx, oracle, D):
    n = 5000
    rng = np.random.default_rng(3 + D)
    corpus = rng.standard_normal((n, D)).astype(np.float32)
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    q = rng.standard_normal((40, D)).astype(np.float32)
    q[:8] = corpus[100:108]  # queries whose best rows get hidden, updated, shown again
    q[8:12] = corpus[2016:2020]  # ... and removed
    s, ref = build(ctx, corpus, ids=ids), build(ctx, corpus, ids=ids, flags=FORBID)

    def same(a, b, qs):
        ra = a.search_vectors(None, 10, qs)
        assert a.last_stats()["screen_bits"] == 6
        rb = b.search_vectors(None, 10, qs)
        assert b.last_stats()["screen_bits"] == 8
        same_hits(ra, rb)
        return ra

    same(s, ref, q)
    hid = ids[96:112]
    for t in (s, ref):
        assert t.hide_items(hid) == 16
    r = same(s, ref, q)
    assert not np.isin(r[0], hid).any()
    corpus[200:216] = (corpus[200:216] * 1e4).astype(np.float32)  # a larger norm: the block scales of their int8 blocks change
    for t in (s, ref):
        t.update_items(ids[200:216], corpus[200:216])
        assert t.unhide_items(hid) == 16
    same(s, ref, q)
    allow = ids[rng.permutation(n)[:2500]]
    v, vr = s.view(allow), ref.view(allow)
    same(v, vr, q)
    v.close()
    vr.close()
    gone = np.unique(np.concatenate([rng.choice(n, 300, replace=False), np.arange(2016, 2048)]))  # scattered rows and block 63 whole
    for t in (s, ref):
        assert t.remove_items(ids[gone]) == gone.size
    r = same(s, ref, q)
    keep = np.setdiff1d(np.arange(n), gone)
    ref_ids, ref_sc = want(oracle, q, corpus[keep], 10, "cosine", ids[keep])
    np.testing.assert_array_equal(r[0], ref_ids)
    np.testing.assert_allclose(r[1], ref_sc, rtol=0, atol=1e-7)
    assert not np.isin(r[0], ids[gone]).any()
    s.close()
    ref.close()
