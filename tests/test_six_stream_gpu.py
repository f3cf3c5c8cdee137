"""GPU: the streaming loop of the 6-bit scan (csrc/scan_kernels.hip, scan_mfma8_kernel with a known chunk count) over waves that
take many blocks.  The loop is written out over lcm(chunks per block, chunk buffers) steps and a wave leaves it at the end of its
last block, wherever in the loop that is; its loader runs buffers - 1 chunks ahead of its multiplies, across block and segment
boundaries and past the end of the stream.  No other small test gives a wave more than three blocks.  With 11 x CUs streaming
waves and (m + 1/2) x 11 x CUs blocks half the waves take m blocks and half m + 1.  Every case runs 64 queries (two query tiles:
three chunk buffers) and 8 (one tile: four), so a wave leaves the loop after its

                                      blocks a wave        64 queries: loop of          8 queries: loop of
    D = 384 (3 chunks)  m = 3, 4, 6   3|4, 4|5, 6|7        1 block: always at its end   4 blocks: after block 3|4, 4|1, 2|3
    D = 256 (2 chunks)  m = 5         5|6                  3 blocks: after block 2|3    2 blocks: after block 1|2
    D = 128 (1 chunk)   m = 5, 8      5|6, 8|9             3 blocks: 2|3, 2|3           4 blocks: 1|2, 4|1

Five segments of unequal size, one of them a single block, cut so that the waves change segment early in their stream (cuts
after 11 x CUs + 1000 blocks and one block on, after 2 x 11 x CUs + 77) and in their last blocks."""
import contextlib

import numpy as np
import pytest

import perceive_amd as pa
import six_ref
from test_six_gpu import FORBID, FORCE, six_bytes
from test_six_paths_gpu import compute_units, same_hits, want

pytestmark = pytest.mark.gpu

CASES = [(384, 3), (384, 4), (384, 6), (256, 5), (128, 5), (128, 8)]


def rows_of(m, stride):
    return (m * stride + stride // 2) * 32 + 9


@pytest.fixture(scope="module")
def corpora():
    """one Gaussian matrix per width, drawn once at the largest m of the width, with its row norms: corpus_of's store"""
    store = {}
    yield store
    store.clear()


def corpus_of(corpora, D, n):
    """the first n rows of the width's matrix, and their norms"""
    if D not in corpora:
        most = rows_of(max(m for d, m in CASES if d == D), 11 * compute_units())
        x = np.random.default_rng(900 + D).standard_normal((most, D), dtype=np.float32)
        corpora[D] = (x, np.sqrt(np.einsum("ij,ij->i", x, x)))
    x, norms = corpora[D]
    return x[:n], norms[:n]


def case_data(corpora, D, m):
    """(corpus, norms, cuts, queries, planted): the rows, where the five segments begin and end, 64 Gaussian queries of which
    three are stored rows"""
    stride = 11 * compute_units()
    n = rows_of(m, stride)
    corpus, norms = corpus_of(corpora, D, n)
    nblk = (n + 31) // 32
    cut_blocks = [0, stride + 1000, stride + 1001, 2 * stride + 77, (m - 1) * stride + 300, nblk]
    assert all(a < b for a, b in zip(cut_blocks, cut_blocks[1:]))
    cuts = [min(32 * b, n) for b in cut_blocks]
    queries = np.random.default_rng(7 * D + m).standard_normal((64, D), dtype=np.float32)
    planted = [n - 1,                                          # the very last block (9 rows)
               32 * ((4 if m >= 4 else m) * stride + 17) + 5,  # wave 17's fifth block (m = 3: its fourth, the last)
               cuts[3] - 1]                                    # the last block in front of a cut
    for q, r in zip((1, 2, 3), planted):
        queries[q] = corpus[r]
    return corpus, norms, cuts, queries, planted


@contextlib.contextmanager
def searchers(ctx, corpus, cuts):
    """the 6-bit searcher and its int8 twin over the same five segments, closed on the way out"""
    pair = []
    try:
        for flags in (FORCE, FORBID):
            x = pa.Searcher(ctx, corpus.shape[1], "cosine")
            pair.append(x)
            x.set_tuning(flags)
            x.set_mid_copy("off")
            for i in range(5):
                x.add_rows(i + 1, corpus[cuts[i] : cuts[i + 1]])
            x.finalize()
            assert x.num_segments == 5
        yield pair
    finally:
        for x in pair:
            x.close()


def approx_scores(queries, corpus, norms):
    return ((queries / np.linalg.norm(queries, axis=1, keepdims=True)) @ corpus.T) / norms[None, :]


@pytest.mark.parametrize("D,m", CASES)
def test_waves_of_many_blocks(ctx, oracle, corpora, D, m):
    """ids and scores are the oracle's (its canonical ranking of each query's 256 best rows by an f32 matrix product: the 10th
    best is far inside them), the hits are bit for bit those of the int8 screen, and the pass streamed every block once."""
    corpus, norms, cuts, queries, planted = case_data(corpora, D, m)
    n = corpus.shape[0]
    ids = np.concatenate([np.arange(cuts[i + 1] - cuts[i], dtype=np.int64) for i in range(5)])  # implicit: the row's number in its source
    approx = approx_scores(queries, corpus, norms)
    ref_ids, ref_sc = np.empty((64, 10), np.int64), np.empty((64, 10), np.float32)
    for q in range(64):
        cand = np.sort(np.argpartition(-approx[q], 256)[:256])  # ascending: the oracle's ties go to the lower position
        assert np.sort(approx[q, cand])[0] < np.sort(approx[q, cand])[-10] - 1e-3
        i, sc = want(oracle, queries[q : q + 1], corpus[cand], 10, "cosine", ids[cand])
        ref_ids[q], ref_sc[q] = i[0], sc[0]
    for q, r in zip((1, 2, 3), planted):
        assert ref_ids[q, 0] == ids[r]
    with searchers(ctx, corpus, cuts) as (s, t):
        for B in (64, 8):
            got = s.search_vectors(None, 10, queries[:B])
            st = s.last_stats()
            assert st["screen_bits"] == 6 and st["scan_launches"] == 1
            assert st["bytes_streamed"] == sum(six_bytes((cuts[i + 1] - cuts[i] + 31) // 32, D) for i in range(5))
            assert st["rows_scanned"] == n
            np.testing.assert_array_equal(got[0], ref_ids[:B])
            np.testing.assert_allclose(got[1], ref_sc[:B], rtol=0, atol=1e-7)
            for q, r in zip((1, 2, 3), planted):
                assert got[0][q, 0] == ids[r]
            twin = t.search_vectors(None, 10, queries[:B])
            assert t.last_stats()["screen_bits"] == 8
            same_hits(got, twin)


def model_counts(corpus, cuts, queries, tau, slack):
    """six_ref.keeps with both tests tightened and loosened by `slack`, summed over the segments a slab of blocks at a time: (lo6,
    lo8), (hi6, hi8).  (Blocks do not depend on one another under cosine.  The codes are small integers, so their products are
    exact in float64 as well, and a float64 product is a BLAS call.)"""
    lo, hi = np.zeros(2, np.int64), np.zeros(2, np.int64)
    for a, b in zip(cuts, cuts[1:]):
        for at in range(a, b, 16384):
            rows = six_ref.Rows(corpus[at : min(at + 16384, b)], "cosine")
            qs = six_ref.Queries(queries, rows)
            rows.u = rows.u.astype(np.float64)
            qs.qh = qs.qh.astype(np.float64)
            lo += [int(x.sum()) for x in six_ref.keeps(rows, qs, tau, -slack)]
            hi += [int(x.sum()) for x in six_ref.keeps(rows, qs, tau, +slack)]
    return tuple(int(x) for x in lo), tuple(int(x) for x in hi)


def range_model(corpus, norms, cuts, queries):
    """the bounds of the fixed-threshold pass and the model's brackets of its two counts, checked for width on the CPU"""
    D = corpus.shape[1]
    approx = approx_scores(queries, corpus, norms)
    bounds = np.ascontiguousarray(-np.partition(-approx, 59, axis=1)[:, 59], dtype=np.float32)
    tau = six_ref.range_tau(bounds, queries, six_ref.Rows(corpus[:32], "cosine"))
    lo, hi = model_counts(corpus, cuts, queries, tau, six_ref.kernel_slack(D))
    print(f"model: 6-bit survivors {lo[0]} .. {hi[0]}, of those past the int8 test {lo[1]} .. {hi[1]}")
    for a, b in zip(lo, hi):
        assert 200 <= a <= b and b - a < 0.02 * a
    return bounds, lo, hi


def test_every_block_is_streamed_once(ctx, corpora):
    """D = 384, m = 4 (waves of 4 and 5 blocks), one range pass: its thresholds never move, so narrow_survivors (rows past the
    6-bit test) and coarse_survivors (of those, the rows past the int8 test) are a function of the copies and the query constants
    alone, and must lie between six_ref.keeps with both tests tightened and loosened by six_ref.kernel_slack(384).  A block
    streamed twice or not at all moves the counts — by one part in the number of blocks each, on average; the bracket is checked
    to be below 2 % wide before the device runs — and no result would show it.  The bound of a query is the f32 cosine of about
    its 60th best row."""
    D, m = 384, 4
    corpus, norms, cuts, queries, _ = case_data(corpora, D, m)
    bounds, (lo6, lo8), (hi6, hi8) = range_model(corpus, norms, cuts, queries)
    with searchers(ctx, corpus, cuts) as (s, t):
        got = s.search_range(None, bounds, queries, 256)
        st = s.last_stats()
        twin = t.search_range(None, bounds, queries, 256)
        st8 = t.last_stats()
    print(f"device: 6-bit survivors {st['narrow_survivors']}, of those past the int8 test {st['coarse_survivors']}; "
          f"int8 screen alone {st8['coarse_survivors']}")
    assert st["screen_bits"] == 6 and st["scan_launches"] == 1 and st8["screen_bits"] == 8 and st8["scan_launches"] == 1
    assert st["rows_scanned"] == corpus.shape[0]
    assert st["bytes_streamed"] == sum(six_bytes((cuts[i + 1] - cuts[i] + 31) // 32, D) for i in range(5))
    assert not got[3].any() and (got[2] >= 20).all() and (got[2] <= 200).all()
    np.testing.assert_array_equal(got[2], twin[2])
    for q in range(64):
        c = int(got[2][q])
        np.testing.assert_array_equal(got[0][q, :c], twin[0][q, :c])
        np.testing.assert_array_equal(got[1][q, :c].view(np.uint32), twin[1][q, :c].view(np.uint32))
    assert lo6 <= st["narrow_survivors"] <= hi6
    assert lo8 <= st["coarse_survivors"] <= hi8
    assert st["coarse_survivors"] <= st8["coarse_survivors"]
