"""GPU: removed items (pcv_searcher_remove_ids).  The yardstick everywhere is a second searcher built fresh from the REMAINING rows
(same source order, row order and hidden set): after a removal every search returns bit for bit what that searcher returns, and
what the oracle returns over the remaining matrix.

The 6-bit screening copy and PCV_MID_COPY_ON exclude each other in the library (the 6-bit copy is never built beside a mid copy
that is ON), so the two are exercised by two cases of test_six_bit_and_mid_copies, not by one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from perceive_amd import _ffi
from perceive_amd.sharded import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

METRIC = {"cosine": 0, "dot": 1}
PCV_ERR_INVALID = 1
FORCE_SIX = 1 << 31


@pytest.fixture(autouse=True)
def small_chunks(monkeypatch):
    # compaction chunks of 1024 rows instead of 2^18, so that these corpora cross chunk boundaries (test_at_size lifts it)
    monkeypatch.setenv("PCV_REMOVE_CHUNK_ROWS", "1024")


@pytest.fixture(scope="module")
def g1000(golden_dir):
    return np.load(os.path.join(golden_dir, "scan_n1000_d384.npz"))


@pytest.fixture(scope="module")
def g77(golden_dir):
    return np.load(os.path.join(golden_dir, "scan_n77_d100.npz"))


def fresh(ctx, dim, metric, parts, screen="auto", mid="off", kernel="auto", tuning=None, hidden=()):
    """A searcher built from scratch: parts = [(source_id, rows, ids or None), ...] in this order."""
    s = pa.Searcher(ctx, dim, metric)
    if len(hidden):
        s.hide_items(np.asarray(hidden, np.int64))  # (the set persists: rows added with these ids are hidden at finalize)
    if tuning is not None:
        s.set_tuning(tuning)
    s.set_screening_copy(screen)
    s.set_mid_copy(mid)
    for src, rows, ids in parts:
        if len(rows):
            s.add_rows(src, rows, ids)
    s.finalize()
    s.set_kernel(kernel)
    return s


def assert_same(a, b):
    """(ids, scores, counts) bit for bit"""
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    np.testing.assert_array_equal(a[2], b[2])


def patterns(n):
    """Rows to remove from a segment of n rows: sparse, a dense run over several blocks (and, from 1100 rows on, over the chunk
    boundary at row 1024), the first and the last row."""
    dense = np.arange(900, 1300) if n >= 1400 else np.arange(n // 4, n // 4 + min(n // 2, 3 * 32 + 7))
    return {"sparse": np.arange(0, n, 7), "dense": dense, "ends": np.array([0, n - 1])}


def check_against_fresh_and_oracle(ctx, oracle, s, corpus, ids, gone_rows, q, metric, ks, **kw):
    keep = np.setdiff1d(np.arange(corpus.shape[0]), gone_rows)
    m, mid = corpus[keep], ids[keep]
    assert s.num_rows == keep.size and s.source_num_rows(1) == keep.size
    f = fresh(ctx, corpus.shape[1], metric, [(1, m, mid)], **kw)
    for k in ks:
        got = s.search_vectors(None, k, q)
        assert_same(got, f.search_vectors(None, k, q))
        opos, _, ocnt = oracle.topk(q, m, k, METRIC[metric])
        np.testing.assert_array_equal(got[2], ocnt)
        for b in range(q.shape[0]):
            np.testing.assert_array_equal(got[0][b, : ocnt[b]], mid[opos[b, : ocnt[b]]])
    rows, rid = s.get_rows(np.arange(keep.size))
    np.testing.assert_array_equal(rows, m)
    np.testing.assert_array_equal(rid, mid)
    f.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("B", [1, 4, 64, 256])
@pytest.mark.parametrize("kernel", ["auto", "wave", "mfma"])
@pytest.mark.parametrize("screen", ["int8", "bf16", "off"])
def test_golden_parity(ctx, oracle, g1000, g77, screen, kernel, B, metric):
    rng = np.random.default_rng(77)
    # the 1000 x 384 fixture with 1600 seeded rows behind it (one segment of 2600 rows: three chunks), and the 77 x 100 fixture
    big = np.concatenate([g1000["corpus"], rng.standard_normal((1600, 384)).astype(np.float32)])
    qbig = np.concatenate([g1000["queries"], rng.standard_normal((192, 384)).astype(np.float32)])[:B]
    qsmall = np.concatenate([g77["queries"], rng.standard_normal((253, 100)).astype(np.float32)])[:B]
    for corpus, q, ks in ((big, qbig, (10, 200)), (g77["corpus"], qsmall, (5, 200))):
        n = corpus.shape[0]
        ids = (40_000 + rng.permutation(n)).astype(np.int64)
        for name, gone in patterns(n).items():
            s = fresh(ctx, corpus.shape[1], metric, [(1, corpus, ids)], screen=screen, kernel=kernel)
            s.search_vectors(None, ks[0], q)
            assert s.remove_items(ids[gone]) == gone.size, name
            check_against_fresh_and_oracle(ctx, oracle, s, corpus, ids, gone, q, metric, ks, screen=screen, kernel=kernel)
            s.close()


@pytest.mark.parametrize("case", ["six", "mid_on"])
def test_six_bit_and_mid_copies(ctx, oracle, g1000, case):
    rng = np.random.default_rng(61)
    corpus = np.concatenate([g1000["corpus"], rng.standard_normal((2200, 384)).astype(np.float32)])
    n = corpus.shape[0]
    ids = np.arange(n, dtype=np.int64) + 100
    q = g1000["queries"][:33]
    kw = dict(tuning=FORCE_SIX, mid="off") if case == "six" else dict(screen="int8", mid="on")
    for metric in ("cosine", "dot"):
        for name, gone in patterns(n).items():
            s = fresh(ctx, 384, metric, [(1, corpus, ids)], **kw)
            s.search_vectors(None, 10, q)
            assert s.remove_items(ids[gone]) == gone.size
            check_against_fresh_and_oracle(ctx, oracle, s, corpus, ids, gone, q, metric, (10, 200), **kw)
            s.search_vectors(None, 10, q)
            st = s.last_stats()
            if case == "six":
                assert st["screening_copy"] == 2 and st["screen_bits"] == 6, (name, st)
            else:
                assert st["screening_copy"] == 2 and st["mid_copy"] == 1, (name, st)
            s.close()


@pytest.mark.parametrize("mid", ["off", "on"])
def test_rows_that_quantise_badly(ctx, oracle, mid):
    rng = np.random.default_rng(15)
    D = 384
    spike = (0.0005 * rng.standard_normal(D)).astype(np.float32)
    spike[0] = 0.9
    near = (spike + 0.005 * rng.standard_normal((6, D))).astype(np.float32)  # near copies (cos ~0.99) raise the threshold
    ids = np.arange(200, dtype=np.int64)
    # case 1: the only spike of block 0 is removed: s_blk of the block grows again
    m = (0.01 * rng.standard_normal((96, D))).astype(np.float32)
    m[5] = spike
    s = fresh(ctx, D, "cosine", [(1, m, ids[:96])], screen="int8", mid=mid, kernel="mfma")
    assert s.remove_items([5]) == 1
    q = np.concatenate([m[[3, 17, 40]], rng.standard_normal((5, D)).astype(np.float32)])
    keep = np.setdiff1d(np.arange(96), [5])
    f = fresh(ctx, D, "cosine", [(1, m[keep], ids[keep])], screen="int8", mid=mid, kernel="mfma")
    got = s.search_vectors(None, 10, q)
    assert_same(got, f.search_vectors(None, 10, q))
    opos, _, _ = oracle.topk(q, m[keep], 10)
    np.testing.assert_array_equal(got[0], ids[keep][opos])
    assert list(got[0][:3, 0]) == [3, 17, 40]
    s.close()
    f.close()
    # case 2: a spike slides into a Gaussian block.  Block 0 holds small Gaussian rows (s_blk far above 127 / 0.9), the spike is row
    # 32 and its near copies rows 64..69; removing row 3 moves the spike to row 31, into block 0.  Its int8 bytes moved along with
    # block 0's old s_blk would clip, and the coarse screen would drop it behind its near copies: the block is packed again, and
    # the spike is the top hit of a query equal to it
    m = (0.01 * rng.standard_normal((128, D))).astype(np.float32)
    m[32] = spike
    m[64:70] = near
    s = fresh(ctx, D, "cosine", [(1, m, ids[:128])], screen="int8", mid=mid, kernel="mfma")
    assert s.remove_items([3]) == 1
    q = np.concatenate([spike[None], rng.standard_normal((7, D)).astype(np.float32)])
    got = s.search_vectors(None, 5, q)
    st = s.last_stats()
    assert st["kernel_used"] == 2 and st["screening_copy"] == 2 and st["mid_copy"] == (1 if mid == "on" else 0)
    assert got[0][0, 0] == 32 and set(got[0][0, 1:]) <= set(range(64, 70))
    assert abs(got[1][0, 0] - 1.0) <= 1e-7
    keep = np.setdiff1d(np.arange(128), [3])
    f = fresh(ctx, D, "cosine", [(1, m[keep], ids[keep])], screen="int8", mid=mid, kernel="mfma")
    assert_same(got, f.search_vectors(None, 5, q))
    opos, _, _ = oracle.topk(q, m[keep], 5)
    np.testing.assert_array_equal(got[0], ids[keep][opos])
    s.close()
    f.close()


def test_many_sources_and_segments(ctx, oracle):
    rng = np.random.default_rng(40)
    D, S = 64, 40
    model = {src: [] for src in range(1, S + 1)}  # source -> [(ids, rows) per add]
    s = pa.Searcher(ctx, D, "cosine")
    s.set_screening_copy("int8")
    next_id = 0
    for rnd in range(3):
        for src in range(1, S + 1):
            n = int(rng.integers(20, 1500)) if src != 9 else 3000  # source 9: adds that open new segments
            ids = np.arange(next_id, next_id + n, dtype=np.int64)
            next_id += n
            if src > 1:  # ids that occur in several sources: some of source 1's first add
                ids[: 5] = model[1][0][0][rnd * 5: rnd * 5 + 5]
            rows = rng.standard_normal((n, D)).astype(np.float32)
            s.add_rows(src, rows, ids)
            model[src].append((ids, rows))
        s.finalize()
    nseg0 = s.num_segments
    assert nseg0 > S
    gone = set(int(x) for x in model[1][0][0][:12])  # shared ids: rows of every source
    gone |= set(int(x) for a in model[7] for x in a[0])  # all of source 7
    gone |= set(int(x) for x in model[9][2][0])  # the whole last add of source 9 (a segment of its own if it opened one)
    gone |= set(int(x) for x in rng.choice(next_id, 4000, replace=False))
    gone_arr = np.array(sorted(gone), np.int64)
    expect = sum(int(np.isin(a[0], gone_arr).sum()) for src in model for a in model[src])
    assert s.remove_items(gone_arr) == expect
    parts, all_ids, all_rows = [], [], []
    for src in range(1, S + 1):
        ids = np.concatenate([a[0] for a in model[src]])
        rows = np.concatenate([a[1] for a in model[src]])
        keep = ~np.isin(ids, gone_arr)
        parts.append((src, rows[keep], ids[keep]))
        assert s.source_num_rows(src) == int(keep.sum())
        all_ids.append(ids[keep])
        all_rows.append(rows[keep])
    assert s.source_num_rows(7) == 0
    all_ids, all_rows = np.concatenate(all_ids), np.concatenate(all_rows)
    assert s.num_rows == all_ids.size
    assert s.num_segments <= nseg0
    rows, rid = s.get_rows(np.arange(all_ids.size))
    np.testing.assert_array_equal(rid, all_ids)
    np.testing.assert_array_equal(rows, all_rows)
    f = fresh(ctx, D, "cosine", parts, screen="int8")
    q = rng.standard_normal((16, D)).astype(np.float32)
    for kernel in ("wave", "mfma"):
        s.set_kernel(kernel)
        f.set_kernel(kernel)
        for filt in (None, [1], [7], [3, 7, 9, 12], [9], list(range(20, 41))):
            for k in (10, 150):
                got = s.search_vectors(filt, k, q)
                assert_same(got, f.search_vectors(filt, k, q))
        got = s.search_vectors(None, 10, q)
        opos, _, _ = oracle.topk(q, all_rows, 10)
        # (ids occur in several sources: compare what the positions carry)
        np.testing.assert_array_equal(got[0], all_ids[opos])
    # the freed tail takes the next rows of a source
    nseg = s.num_segments
    more = rng.standard_normal((10, D)).astype(np.float32)
    mid = np.arange(next_id, next_id + 10, dtype=np.int64)
    s.add_rows(3, more, mid)
    s.finalize()
    assert s.num_segments == nseg
    f.add_rows(3, more, mid)
    f.finalize()
    assert_same(s.search_vectors(None, 10, more), f.search_vectors(None, 10, more))
    s.close()
    f.close()


def test_implicit_ids(ctx, oracle):
    rng = np.random.default_rng(23)
    D = 384
    # add_rows(ids=None): ids = row numbers; add_synthetic: ids = first_row + row, no id column until a row goes
    m = rng.standard_normal((3000, D)).astype(np.float32)
    q = rng.standard_normal((8, D)).astype(np.float32)
    for gone in (np.arange(1200, 1500), np.arange(0, 40), np.arange(2950, 3000), np.array([5, 1024, 2999])):
        s = fresh(ctx, D, "cosine", [(1, m, None)])
        assert s.remove_items(gone) == gone.size
        check_against_fresh_and_oracle(ctx, oracle, s, m, np.arange(3000, dtype=np.int64), gone, q, "cosine", (10,))
        s.close()
    ref = oracle.synth_rows(0x52, 100, 5000, D)
    sid = np.arange(100, 5100, dtype=np.int64)
    for gone in (np.arange(2000, 2600), np.arange(100, 164), np.arange(5000, 5100), np.array([99, 117, 4100, 5100, 5099])):
        s = pa.Searcher(ctx, D, "cosine")
        s.add_synthetic(1, 5000, 0x52, first_row=100)
        s.finalize()
        hit = gone[(gone >= 100) & (gone < 5100)]
        assert s.remove_items(gone) == hit.size
        keep = ~np.isin(sid, hit)
        rows, rid = s.get_rows(np.arange(int(keep.sum())))
        np.testing.assert_array_equal(rid, sid[keep])
        np.testing.assert_array_equal(rows, ref[keep])
        f = fresh(ctx, D, "cosine", [(1, ref[keep], sid[keep])])
        for k in (10, 200):
            got = s.search_vectors(None, k, q)
            assert_same(got, f.search_vectors(None, k, q))
        opos, _, _ = oracle.topk(q, ref[keep], 10)
        np.testing.assert_array_equal(s.search_vectors(None, 10, q)[0], sid[keep][opos])
        s.close()
        f.close()
    # every row of a synthetic segment
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, 500, 0x52)
    s.add_rows(2, m[:100], np.arange(9000, 9100, dtype=np.int64))
    s.finalize()
    assert s.remove_items(np.arange(0, 500)) == 500
    assert s.num_rows == 100 and s.source_num_rows(1) == 0 and s.num_segments == 1
    f = fresh(ctx, D, "cosine", [(2, m[:100], np.arange(9000, 9100, dtype=np.int64))])
    assert_same(s.search_vectors(None, 10, q), f.search_vectors(None, 10, q))
    s.close()
    f.close()


def test_interplay_with_hide_update_and_add(ctx, oracle):
    rng = np.random.default_rng(29)
    N, D = 4000, 128
    m = rng.standard_normal((N, D)).astype(np.float32)
    ids = (rng.permutation(3 * N)[:N]).astype(np.int64)
    q = rng.standard_normal((16, D)).astype(np.float32)
    kw = dict(screen="int8", mid="on")

    def same_as_fresh(s, rows, rid, hidden=()):
        f = fresh(ctx, D, "cosine", [(1, rows, rid)], hidden=hidden, **kw)
        for kernel in ("wave", "mfma"):
            s.set_kernel(kernel)
            f.set_kernel(kernel)
            for k in (10, 200):
                assert_same(s.search_vectors(None, k, q), f.search_vectors(None, k, q))
        assert s.hidden_rows == f.hidden_rows
        f.close()

    s = fresh(ctx, D, "cosine", [(1, m, ids)], **kw)
    top = s.search_vectors(None, 3, q)[0]
    hid = np.unique(np.concatenate([top[:, 0], ids[1000:1040]]))
    assert s.hide_items(hid) == hid.size
    # hide, then remove other ids (and two hidden ones), then unhide
    gone_at = np.setdiff1d(np.concatenate([np.arange(50, 2500, 9), np.arange(3000, 3100)]), np.flatnonzero(np.isin(ids, hid)))
    gone = np.concatenate([ids[gone_at], hid[:2]])
    assert s.remove_items(gone) == gone.size
    keep = ~np.isin(ids, gone)
    assert s.hidden_rows == hid.size - 2
    same_as_fresh(s, m[keep], ids[keep], hidden=hid)
    assert s.unhide_items(hid[2:]) == hid.size - 2
    same_as_fresh(s, m[keep], ids[keep], hidden=hid[:2])
    # a removed hidden id comes back with a new row: hidden at finalize, because the set persists
    v = q[:1].copy()
    s.add_rows(1, v, hid[:1])
    s.finalize()
    assert s.hidden_rows == 1
    rows2, ids2 = np.concatenate([m[keep], v]), np.concatenate([ids[keep], hid[:1]])
    same_as_fresh(s, rows2, ids2, hidden=hid[:2])
    assert s.search_vectors(None, 1, v)[0][0, 0] != hid[0]
    # update after remove
    upd_at = rng.choice(ids2.size - 1, 300, replace=False)
    vecs = rng.standard_normal((300, D)).astype(np.float32)
    found, changed = s.update_items(ids2[upd_at], vecs)
    assert found.all() and changed == 300
    rows2 = rows2.copy()
    rows2[upd_at] = vecs
    same_as_fresh(s, rows2, ids2, hidden=hid[:2])
    # remove twice in a row, then add rows into the freed tail
    nseg = s.num_segments
    for part in (ids2[5:400:3], ids2[2000:2300]):
        assert s.remove_items(part) == part.size
        k2 = ~np.isin(ids2, part)
        rows2, ids2 = rows2[k2], ids2[k2]
        same_as_fresh(s, rows2, ids2, hidden=hid[:2])
    more = rng.standard_normal((200, D)).astype(np.float32)
    mid = np.arange(50_000, 50_200, dtype=np.int64)
    s.add_rows(1, more, mid)
    s.finalize()
    assert s.num_segments == nseg
    rows2, ids2 = np.concatenate([rows2, more]), np.concatenate([ids2, mid])
    same_as_fresh(s, rows2, ids2, hidden=hid[:2])
    # ids that match nothing
    before = s.search_vectors(None, 10, q)
    assert s.remove_items(np.array([-1, 10**12, int(gone[0])], np.int64)) == 0
    assert s.num_rows == ids2.size
    assert_same(s.search_vectors(None, 10, q), before)
    assert s.remove_items(np.zeros(0, np.int64)) == 0
    s.close()


def hits_of(ctx, fn, B, k):
    n = B * k * HIT_DTYPE.itemsize
    d = ctx.alloc(n)
    try:
        fn(d)
        return ctx.to_host(d, n).view(HIT_DTYPE)
    finally:
        ctx.free(d)


def test_views_follow_a_removal(ctx, oracle, g1000):
    rng = np.random.default_rng(33)
    corpus = np.concatenate([g1000["corpus"], rng.standard_normal((1500, 384)).astype(np.float32)])
    n = corpus.shape[0]
    ids = (rng.permutation(n) + 20_000).astype(np.int64)
    q = g1000["queries"]
    allow = rng.choice(ids, 900, replace=False)
    for metric in ("cosine", "dot"):
        s = fresh(ctx, 384, metric, [(1, corpus, ids)], screen="int8")
        s.set_shard_offset(1000)
        v = s.view(allow)
        v.search_vectors(None, 10, q)
        gone = np.concatenate([allow[:300], ids[np.arange(0, n, 11)]])
        removed = s.remove_items(gone)
        assert removed == np.unique(gone).size
        keep = ~np.isin(ids, gone)
        in_view = keep & np.isin(ids, allow)
        f = fresh(ctx, 384, metric, [(1, corpus[in_view], ids[in_view])], screen="int8")
        for k in (10, 200):
            assert_same(v.search_vectors(None, k, q), f.search_vectors(None, k, q))
        assert v.view_stats()["rows"] == int(in_view.sum()) and v.view_stats()["refreshes"] == 1
        pos_of = {int(i): 1000 + p for p, i in enumerate(ids[keep])}  # the parent's NEW positions
        h = hits_of(ctx, lambda d: v.search_device(None, 10, q, d), 64, 10)
        ok = h["pos"] >= 0
        assert ok.sum() == 640
        assert all(pos_of[int(i)] == int(x) for i, x in zip(h["id"][ok], h["pos"][ok]))
        hp = hits_of(ctx, lambda d: s.search_device(None, 10, q, d), 64, 10)
        assert all(pos_of[int(i)] == int(x) for i, x in zip(hp["id"], hp["pos"]))
        v.close()
        s.close()
        f.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_replayed_pass_sees_the_removal(ctx, oracle, metric):
    rng = np.random.default_rng(3)
    m = rng.standard_normal((5000, 384)).astype(np.float32)
    q = rng.standard_normal((16, 384)).astype(np.float32)
    s = fresh(ctx, 384, metric, [(1, m, None)], screen="int8")
    for _ in range(4):  # the same pass shape again and again: captured as a graph and replayed
        first = s.search_vectors(None, 10, q)
    # the best hit of every query goes, with a few other rows
    gone = np.unique(np.concatenate([first[0][:, 0], rng.choice(5000, 10, replace=False)]))
    assert s.remove_items(gone) == gone.size
    keep = np.setdiff1d(np.arange(5000), gone)
    ids, sc, cnt = s.search_vectors(None, 10, q)
    opos, _, ocnt = oracle.topk(q, m[keep], 10, METRIC[metric])
    np.testing.assert_array_equal(ids, keep[opos])
    np.testing.assert_array_equal(cnt, ocnt)
    f = fresh(ctx, 384, metric, [(1, m[keep], keep.astype(np.int64))], screen="int8")
    for _ in range(4):
        assert_same(s.search_vectors(None, 10, q), f.search_vectors(None, 10, q))
    s.close()
    f.close()


def test_refusals(ctx):
    rng = np.random.default_rng(11)
    D = 64
    m = rng.standard_normal((500, D)).astype(np.float32)
    q = rng.standard_normal((4, D)).astype(np.float32)
    s = fresh(ctx, D, "cosine", [(1, m, np.arange(500, dtype=np.int64))])
    before = s.search_vectors(None, 10, q)
    v = s.view(np.arange(100, dtype=np.int64))
    with pytest.raises(_ffi.PcvError) as e:
        v.remove_items([3, 4])  # a view is read-only
    assert e.value.status == PCV_ERR_INVALID
    v.close()
    s.add_rows(1, m[:1], np.array([900], np.int64))  # pending rows
    with pytest.raises(_ffi.PcvError) as e:
        s.remove_items([3, 4])
    assert e.value.status == PCV_ERR_INVALID
    s.finalize()
    assert s.num_rows == 501
    before = s.search_vectors(None, 10, q)
    out = ctx.alloc(4 * 10 * 24 + 64)
    s.search_device_begin(None, 10, q, out)  # a queued pass
    with pytest.raises(_ffi.PcvError) as e:
        s.remove_items([3, 4])
    assert e.value.status == PCV_ERR_INVALID
    s.search_device_end()
    ctx.free(out)
    lib = _ffi.lib()
    n = C.c_int64(7)
    assert lib.pcv_searcher_remove_ids(s._handle, None, 3, C.byref(n)) == PCV_ERR_INVALID
    assert lib.pcv_searcher_remove_ids(s._handle, _ffi.i64p(np.arange(3, dtype=np.int64)), -1, C.byref(n)) == PCV_ERR_INVALID
    assert s.num_rows == 501
    assert_same(s.search_vectors(None, 10, q), before)
    rows, rid = s.get_rows(np.array([3, 4, 500]))
    np.testing.assert_array_equal(rid, [3, 4, 900])
    assert lib.pcv_searcher_remove_ids(s._handle, _ffi.i64p(np.array([3, 3, 4], np.int64)), 3, None) == 0  # out_rows may be NULL
    assert s.num_rows == 499
    s.close()


def _free_bytes(ctx):
    # hipMemGetInfo of libamdhip64.so, looked up through the library's own handle: the HIP runtime the library allocates with.
    # (By name, dlopen may hand back another copy of the runtime that an earlier test's imports loaded; it knows no device.)
    hip = C.CDLL(_ffi.LIB_PATH)
    free, total = C.c_size_t(), C.c_size_t()
    ctx.synchronize()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_device_memory_is_given_back(ctx, monkeypatch):
    monkeypatch.delenv("PCV_REMOVE_CHUNK_ROWS")  # the chunk the library uses by itself
    SLACK = 64 << 20
    N, D = 600_000, 384
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, N, 0x77)  # implicit ids: the removal gives the segment an id column
    s.add_synthetic(2, N, 0x78, first_row=10_000_000)
    s.finalize()
    rng = np.random.default_rng(2)
    free0 = _free_bytes(ctx)
    gone = rng.choice(N, 50_000, replace=False)
    assert s.remove_items(gone) == gone.size
    free1 = _free_bytes(ctx)
    id_column = (N + 31) // 32 * 32 * 8
    assert free0 - free1 <= id_column + SLACK, (free0, free1)
    # a second removal from the same segment needs no new id column
    gone2 = np.setdiff1d(rng.choice(N, 50_000, replace=False), gone)
    assert s.remove_items(gone2) == gone2.size
    free2 = _free_bytes(ctx)
    assert free1 - free2 <= SLACK, (free1, free2)
    # a removal that empties a segment gives its rows back
    assert s.remove_items(np.arange(10_000_000, 10_000_000 + N)) == N
    free3 = _free_bytes(ctx)
    assert free3 - free2 >= N * D * 4, (free2, free3)
    assert s.num_rows == N - gone.size - gone2.size and s.source_num_rows(2) == 0
    s.close()


def _verify_topk(searcher, oracle, q, ids, pos, sc, k, n_total, rng, sample=256):
    """test_update_gpu.py::_verify_topk: scores re-derived by the oracle from the rows read back at the hits' positions `pos`,
    list sorted, and a random sample of other rows never beats the k-th score unless it is in the list."""
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
    return sids


def test_at_size(ctx, oracle, monkeypatch):
    # 10M synthetic rows (implicit ids = positions); 1M random ids and the run [4 000 000, 4 100 000) go.  Rows planted right in
    # front of and right behind the run (and at the segment's ends) must come back as the best hit of their own vector, at their new
    # position; this is the one test that samples (256 rows per _verify_topk, as test_update_gpu.py does)
    monkeypatch.delenv("PCV_REMOVE_CHUNK_ROWS")
    N, D, k, SEED = 10_000_000, 384, 10, 0x5E8
    RUN0, RUN1 = 4_000_000, 4_100_000
    rng = np.random.default_rng(14)
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, N, SEED)
    s.finalize()
    plant_ids = np.concatenate([np.arange(RUN0 - 40, RUN0), np.arange(RUN1, RUN1 + 40), [0, 1, N - 2, N - 1]]).astype(np.int64)
    planted = rng.standard_normal((plant_ids.size, D), dtype=np.float32)
    found, changed = s.update_items(plant_ids, planted)
    assert found.all() and changed == plant_ids.size
    gone = np.setdiff1d(np.concatenate([rng.choice(N, 1_000_000, replace=False), np.arange(RUN0, RUN1)]), plant_ids).astype(np.int64)
    assert s.remove_items(gone) == gone.size
    assert s.num_rows == N - gone.size and s.source_num_rows(1) == N - gone.size

    def pos_of(x):  # new position of a remaining id: the removed ids below it are gone
        return x - np.searchsorted(gone, x)

    back, bid = s.get_rows(pos_of(plant_ids))
    np.testing.assert_array_equal(bid, plant_ids)
    np.testing.assert_array_equal(back, planted)
    res = []
    for c in range(0, plant_ids.size, 64):
        res.append(s.search_vectors(None, k, planted[c: c + 64]))
    ids = np.concatenate([r[0] for r in res])
    sc = np.concatenate([r[1] for r in res])
    cnt = np.concatenate([r[2] for r in res])
    assert (cnt == k).all()
    np.testing.assert_array_equal(ids[:, 0], plant_ids)  # every planted row, exhaustively
    assert (np.abs(sc[:, 0] - 1.0) <= 1e-6).all()
    assert not np.isin(ids, gone).any()
    sub = rng.choice(plant_ids.size, 16, replace=False)
    sids = _verify_topk(s, oracle, planted[sub], ids[sub], pos_of(ids[sub]), sc[sub], k, N - gone.size, rng)
    assert not np.isin(sids, gone).any()
    # rows read back around the run are the generator's rows of their ids
    around = np.array([RUN0 - 41, RUN1 + 40, RUN1 + 41], np.int64)
    around = around[~np.isin(around, gone)]
    rows, rid = s.get_rows(pos_of(around))
    np.testing.assert_array_equal(rid, around)
    for i, x in enumerate(around):
        np.testing.assert_array_equal(rows[i], oracle.synth_rows(SEED, int(x), 1, D)[0])
    s.close()


def test_cpp_mirror_removes_on_gpu():
    src = os.path.join(ROOT, "tests", "cpp", "remove_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "remove_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "remove_mirror_test: ok" in r.stdout
