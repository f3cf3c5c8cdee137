"""The searcher's pass pipeline (csrc/searcher_pass.cpp: enqueue_pass / finish_pass) seen through the C ABI: a pass gives the same hits
and books the same statistics whether its launches are queued plainly, captured into a graph (the third sighting of a shape) or
replayed; every kind of pass shares one workspace without leaving anything behind for the next; and the numeric PCV_SCAN_FLAGS
words keep their meaning.  Expected hits come from the oracle, expected byte counts from the layout documented in csrc/scan.h."""
import numpy as np
import pytest

import perceive_amd as pa
from test_range_gpu import Ranking, check
from test_scan_gpu import build, guess_breaking_rows
from test_six_gpu import FORBID, FORCE
from test_six_gpu import build as build_six
from test_view_gpu import hits_of

pytestmark = pytest.mark.gpu

MODES = {"off": 0, "bf16": 1, "int8": 2}
SAME_STATS = ("rows_scanned", "scan_launches", "kernel_used", "screening_copy", "screen_bits", "mid_copy", "bytes_streamed")
# Scores are the canonical f64 score rounded to f32 on both sides; the two f64 sums may differ in their last bits, so the f32
# values differ by at most one f32 ulp of a cosine (|c| <= 1): 2^-24 = 6e-8.
ATOL = 1e-7


def block_bytes(D, mode):
    """bytes the scan streams per 32-row block (csrc/scan.h): f32 pieces + 32 row scales; bf16 pieces; int8 pieces + one scale"""
    Dp, Dp8 = (D + 63) // 64 * 64, (D + 127) // 128 * 128
    return {"off": Dp * 4 * 32 + 128, "bf16": Dp * 2 * 32, "int8": Dp8 * 32 + 4}[mode]


def six_times_the_same(s, q, k, mode, want_pos, want_scores, nrows, D):
    """plain, plain, capture on the third sighting of the shape, then replays.  The C ABI has no word that says whether a pass was
    replayed, so nothing here shows that a capture took place: the test holds what a caller can see — hits and statistics — to the
    same values over the calls in which the searcher changes how it queues the pass.
    The mid copy is switched off by the callers: at these sizes the survivors' f32 rows are a visible share of a pass, so AUTO
    would build the copy beside the searches after two passes (searcher_pass.cpp: note_mid_trigger) and `mid_copy` would change from
    0 to 1 part way through the six calls — by design, and nothing to do with how the pass is queued."""
    first_ids = first_scores = first_stats = None
    for run in range(6):
        ids, scores, counts = s.search_vectors(None, k, q)
        st = s.last_stats()
        stats = {f: st[f] for f in SAME_STATS}
        print(run, mode, q.shape[0], stats)
        if run == 0:
            first_ids, first_scores, first_stats = ids, scores, stats
            np.testing.assert_array_equal(ids, want_pos)
            np.testing.assert_allclose(scores, want_scores.astype(np.float32), rtol=0, atol=ATOL)
            assert (counts == k).all()
            assert st["scan_launches"] == 1 and st["rows_scanned"] == nrows and st["screening_copy"] == (MODES[mode] if st["kernel_used"] == 2 else 0)
            streamed = mode if st["kernel_used"] == 2 else "off"  # (the wave kernel reads the f32 rows whatever copies there are)
            assert st["bytes_streamed"] == (nrows + 31) // 32 * block_bytes(D, streamed)
            assert st["screen_bits"] == (8 if st["screening_copy"] == 2 else 0) and st["mid_copy"] == 0
        else:
            np.testing.assert_array_equal(ids, first_ids)
            np.testing.assert_array_equal(scores.view(np.uint32), first_scores.view(np.uint32))
            assert stats == first_stats, (run, stats, first_stats)
    return first_stats


@pytest.fixture(scope="module")
def synth3000(oracle):
    N, D, k = 3000, 384, 10
    rows = oracle.synth_rows(0x5EED, 0, N, D)
    q = oracle.synth_rows(0x5EED + 1, 0, 64, D)
    pos, sc, _ = oracle.topk(q, rows, k)
    return rows, q, k, pos, sc


@pytest.mark.parametrize("mode", ["off", "bf16", "int8"])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_replay_changes_nothing(ctx, synth3000, mode, B):
    rows, q, k, pos, sc = synth3000
    s = pa.Searcher(ctx, rows.shape[1], "cosine")
    s.set_screening_copy(mode)
    s.set_mid_copy("off")
    s.add_synthetic(1, rows.shape[0], 0x5EED)
    s.finalize()
    st = six_times_the_same(s, q[:B], k, mode, pos[:B], sc[:B], rows.shape[0], rows.shape[1])
    # with copies the MFMA kernel streams fewer bytes whatever the batch; without, up to four queries go to the wave kernel
    assert st["kernel_used"] == (1 if mode == "off" and B <= 4 else 2)
    s.close()


@pytest.mark.parametrize("mode", ["off", "bf16", "int8"])
def test_replay_at_an_awkward_width(ctx, oracle, golden_dir, mode):
    # 77 rows of 100 features: Dp = 128, two blocks and a partial one, three queries
    import os

    g = np.load(os.path.join(golden_dir, "scan_n77_d100.npz"))
    rows, q, k = g["corpus"], g["queries"], int(g["k"])
    assert rows.shape == (77, 100) and q.shape[0] == 3
    pos, sc, _ = oracle.topk(q, rows, k)
    np.testing.assert_array_equal(pos, g["topk_f64"])
    s = build(ctx, rows, screen=mode)
    s.set_mid_copy("off")
    st = six_times_the_same(s, q, k, mode, pos, sc, 77, 100)
    assert st["kernel_used"] == (1 if mode == "off" else 2)  # the wave kernel where there is no copy to stream
    s.close()


def test_every_pass_kind_through_one_searcher(ctx, oracle):
    N, D, B = 2000, 384, 5
    rows = oracle.synth_rows(0xA11, 0, N, D)
    q = oracle.synth_rows(0xA12, 0, B, D)
    ids = np.arange(N, dtype=np.int64)
    rank = Ranking(oracle, q, rows, ids, "cosine")  # the canonical order of every row, once
    s = pa.Searcher(ctx, D, "cosine")
    s.set_screening_copy("int8")
    s.add_synthetic(1, N, 0xA11)
    s.finalize()

    def top(k):
        got_ids, got_sc, cnt = s.search_vectors(None, k, q)
        assert (cnt == k).all()
        np.testing.assert_array_equal(got_ids, rank.pos[:, :k])
        np.testing.assert_allclose(got_sc, rank.scores[:, :k], rtol=0, atol=ATOL)
        return got_ids, got_sc

    first = top(10)
    assert s.last_stats()["scan_launches"] == 1 and s.last_stats()["screening_copy"] == 2
    top(300)  # 128 + 128 + 44 under ceilings
    assert s.last_stats()["scan_launches"] == 3
    # a bound that admits about 700 rows per query, from the oracle's sorted scores
    bounds = rank.scores[:, 699].copy()
    got = s.search_range(None, bounds, q, N)
    for b in range(B):
        wi, ws = rank.expect(b, bounds[b])
        assert 700 <= len(wi) < 720
        check(got, wi, ws, b, N)  # (ids, and scores bit for bit: a range result is a cut top-k result)
    k = 10
    h = hits_of(ctx, lambda d: s.search_device(None, k, q, d), B, k)
    np.testing.assert_array_equal(h["pos"].reshape(B, k), rank.pos[:, :k])
    np.testing.assert_array_equal(h["id"].reshape(B, k), rank.pos[:, :k])
    np.testing.assert_allclose(h["score"].reshape(B, k).astype(np.float32), rank.scores[:, :k], rtol=0, atol=ATOL)
    over = []
    hb = hits_of(ctx, lambda d: (s.search_device_begin(None, k, q, d), over.append(s.search_device_end())), B, k, extra=1)
    assert over == [False] and int(hb["pos"][B * k]) == 0  # a clear overflow record behind the hits
    np.testing.assert_array_equal(hb["pos"][: B * k].reshape(B, k), rank.pos[:, :k])
    np.testing.assert_allclose(hb["score"][: B * k].reshape(B, k).astype(np.float32), rank.scores[:, :k], rtol=0, atol=ATOL)
    again = s.search_vectors(None, 10, q)
    np.testing.assert_array_equal(again[0], first[0])
    np.testing.assert_array_equal(again[1].view(np.uint32), first[1].view(np.uint32))
    s.close()


def test_flag_words_keep_their_meaning(ctx, oracle, golden_dir):
    import os

    # 32: no speculative start threshold.  On the rows on which a guess must fail, a FRESH searcher told so before its first search
    # needs no repeat (after a failed guess the searcher holds guesses back for a while by itself, whatever the word says)
    m, q, k, _seed_rows, _other_rows, _rng = guess_breaking_rows()
    s = build(ctx, m, kernel="mfma")
    s.set_tuning(32)
    ids, scores, _ = s.search_vectors(None, k, q)
    st = s.last_stats()
    assert st["speculation_reruns"] == 0 and st["scan_launches"] == 1 and st["screening_copy"] == 2, st
    opos, osc, _ = oracle.topk(q, m, k)
    np.testing.assert_array_equal(ids, opos)
    np.testing.assert_allclose(scores, osc.astype(np.float32), rtol=0, atol=ATOL)
    s.close()
    s = build(ctx, m, kernel="mfma")  # (the rows do what they are made for: without the word the guess fails once)
    s.search_vectors(None, k, q)
    st = s.last_stats()
    assert st["speculation_reruns"] == 1 and st["scan_launches"] == 2, st
    s.close()
    # 1 << 29: never the 6-bit copy; 1 << 31: AUTO builds it at any size (and the pass streams it)
    assert (FORBID, FORCE) == (0x20000000, 0x80000000)
    g = np.load(os.path.join(golden_dir, "scan_n1000_d384.npz"))
    s = build_six(ctx, g["corpus"])  # forced to six-bit copies at 1000 rows
    q16 = g["queries"][:16]
    s.set_tuning(1 << 29)
    s.search_vectors(None, 10, q16)
    assert s.last_stats()["screen_bits"] == 8
    s.set_tuning(1 << 31)
    s.search_vectors(None, 10, q16)
    assert s.last_stats()["screen_bits"] == 6
    s.close()
