"""GPU: diverse results (pcv_searcher_search_diverse), through the C ABI via the Python mirror.  The reference of every check is
tests/diverse_ref.py: oracle.topk over all rows gives the ranked list, and the greedy MMR walk runs over it in Python floats with
orc_canonical_score as the pair cosine.  Ids, ranks, counts, examined and exact are compared for equality, scores as f32 bits,
marginal values as f64 bits, and the fill values behind the picks."""
import os
import subprocess

import numpy as np
import pytest

import diverse_ref as dr
import perceive_amd as pa
from diverse_ref import Reference, bits32, check, default_pool, planted_corpus, planted_queries
from test_diverse_cpu import CERT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384
FORCE_SIX = 1 << 31
SPLIT = dr.SPLIT
FORMS = {
    "wave": ("wave", "off", "off", 0),
    "mfma_int8": ("mfma", "int8", "off", 0),
    "auto_six": ("auto", "auto", "off", FORCE_SIX),
}
LAMBDAS = (1.0, 0.7, 0.5, 0.0)


def build_three_segments(ctx, metric, rows, ids, form, dim=D):
    s = pa.Searcher(ctx, dim, metric)
    kernel, copy, mid, tuning = form
    s.set_kernel(kernel)
    s.set_screening_copy(copy)
    s.set_mid_copy(mid)
    s.set_tuning(tuning)
    a, b = SPLIT
    s.add_rows(1, rows[:a], ids[:a])
    s.finalize()
    s.add_rows(1, rows[a:b], ids[a:b])
    s.add_rows(2, rows[b:], ids[b:])
    s.finalize()
    assert s.num_segments >= 3 and s.num_rows == rows.shape[0]
    return s


@pytest.fixture(scope="module")
def planted(oracle):
    out = {}
    for metric in ("cosine", "dot"):
        rows, ids, anchors = planted_corpus(metric, D)
        queries = planted_queries(metric, anchors, D)
        out[metric] = (rows, ids, queries, Reference(oracle, queries, rows, ids, metric))
    return out


# ---- 1. planted families, three screen forms, both metrics ---------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("form", list(FORMS))
def test_planted_families(ctx, planted, form, metric):
    rows, ids, queries, ref = planted[metric]
    s = build_three_segments(ctx, metric, rows, ids, FORMS[form])
    for B in (1, 3, 16):
        for k in (1, 10, 128):
            for lam in LAMBDAS:
                got = s.search_diverse(None, k, queries[:B], lam)
                for q in range(B):
                    check(got, ref.walk(q, k, lam, default_pool(k)), q, k)
    # a source filter: only the rows of source 2; a pool that is no multiple of the pass's 128 hits or of the workgroup
    allowed = np.arange(SPLIT[1], rows.shape[0])
    got = s.search_diverse([2], 10, queries, 0.5, pool=200)
    for q in range(16):
        check(got, ref.walk(q, 10, 0.5, 200, allowed), q, 10)
    empty = s.search_diverse([], 10, queries[:3], 0.5)  # an empty filter matches nothing: the list ended inside the pool
    assert (empty[4] == 0).all() and (empty[5] == 0).all() and empty[6].all()
    assert (empty[0] == -1).all() and np.isnan(empty[1]).all() and np.isnan(empty[2]).all() and (empty[3] == -1).all()
    s.close()
    # The families were skipped: at lambda = 0.5 an anchor query leaves the ranks of its anchor's families (about 70 rows) behind.
    # Under the dot metric relevance is c / dim, of the size of the row's amplitude, and ten picks stay nearer the head of the list:
    # there the ten picks skip ranks (they are not 0..9) and the 128 picks reach far beyond rank 20.
    for q in range(8):
        ten, many = ref.walk(q, 10, 0.5, default_pool(10)), ref.walk(q, 128, 0.5, default_pool(128))
        assert many.ranks.max() >= 20
        assert ten.ranks.max() >= (20 if metric == "cosine" else 10)


# ---- 2. lambda = 1 is the plain search -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_lambda_one_is_the_plain_top_k(ctx, planted, metric):
    rows, ids, queries, _ref = planted[metric]
    s = build_three_segments(ctx, metric, rows, ids, ("auto", "auto", "auto", 0))
    for k in (1, 10, 128):
        plain = s.search_vectors(None, k, queries)
        got = s.search_diverse(None, k, queries, 1.0)
        np.testing.assert_array_equal(got[0], plain[0])
        np.testing.assert_array_equal(bits32(got[1]), bits32(plain[1]))
        np.testing.assert_array_equal(got[3], np.tile(np.arange(k, dtype=np.int32), (16, 1)))
        assert (got[4] == k).all() and (got[5] == default_pool(k)).all()
    s.close()


# ---- 3. widths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [100, 768, 2048])
def test_widths(ctx, oracle, dim):
    """dim 100: padded rows, no multiple of 128 or of 16; 768 and 2048: more than one piece per lane in the gather"""
    rows, ids, anchors = planted_corpus("cosine", dim, seed=12, n_base=500, families=((0.999, 9), (0.97, 9), (0.9, 5)), n_anchor=3)
    queries = planted_queries("cosine", anchors, dim)[:4]
    ref = Reference(oracle, queries, rows, ids, "cosine")
    s = pa.Searcher(ctx, dim, "cosine")
    s.add_rows(1, rows, ids)
    s.finalize()
    for k, pool in ((10, 128), (40, 200), (128, 300)):
        for lam in (0.7, 0.3):
            got = s.search_diverse(None, k, queries, lam, pool=pool)
            for q in range(4):
                check(got, ref.walk(q, k, lam, pool), q, k)
    assert ref.walk(0, 10, 0.3, 128).ranks.max() >= 20
    s.close()


# ---- 4. several passes ---------------------------------------------------------------------------------------------------------
def test_several_passes_and_a_clean_scan_state(ctx, planted):
    rows, ids, queries, ref = planted["cosine"]
    s = build_three_segments(ctx, "cosine", rows, ids, ("auto", "auto", "auto", 0))
    qs = queries[[0, 1, 8, 9, 12]]
    before = s.search_vectors(None, 10, qs)
    got = s.search_diverse(None, 5, qs, 0.5, pool=1024)
    st = s.last_stats()
    for i, q in enumerate((0, 1, 8, 9, 12)):
        want = ref.walk(q, 5, 0.5, 1024)
        check((got[0][i : i + 1], got[1][i : i + 1], got[2][i : i + 1], got[3][i : i + 1], got[4][i : i + 1], got[5][i : i + 1], got[6][i : i + 1]),
              want, 0, 5)
    assert (got[5] == 1024).all()
    assert st["scan_launches"] >= (1024 + 127) // 128  # one scan per pass of 128 hits: nothing stops a query early
    assert st["scan_launches"] <= (1024 + 127) // 128 + 2  # (a pass is repeated where a candidate list overflows or a guess fails)
    after = s.search_vectors(None, 10, qs)  # the scan state was left clean
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(bits32(after[1]), bits32(before[1]))
    s.close()


# ---- 5. more than one group of queries -----------------------------------------------------------------------------------------
def test_more_than_one_query_group(ctx, oracle):
    rng = np.random.default_rng(31)
    N, B = 600, 70
    rows = rng.standard_normal((N, D)).astype(np.float32)
    rows[300:360] = (rows[:60] + 0.2 * rng.standard_normal((60, D))).astype(np.float32)  # near copies: something to skip
    ids = (rng.permutation(N) * 3 + 11).astype(np.int64)
    queries = (rows[rng.integers(0, 60, B)] + 0.1 * rng.standard_normal((B, D))).astype(np.float32)
    ref = Reference(oracle, queries, rows, ids, "cosine")
    assert any(ref.walk(q, 10, 0.5, 128).ranks[1] != 1 for q in range(B))
    # the wave kernel takes 4 queries a pass: 18 groups, the last of two queries; the default form as many as its scan takes
    for kernel in ("wave", "auto"):
        s = pa.Searcher(ctx, D, "cosine")
        s.set_kernel(kernel)
        s.add_rows(1, rows, ids)
        s.finalize()
        got = s.search_diverse(None, 10, queries, 0.5, pool=128)
        for q in range(B):
            check(got, ref.walk(q, 10, 0.5, 128), q, 10)
        for q in (0, B - 1):
            alone = s.search_diverse(None, 10, queries[q : q + 1], 0.5, pool=128)
            for a, b in zip(alone, got):
                np.testing.assert_array_equal(np.atleast_1d(a[0]).view(np.uint8), np.atleast_1d(b[q]).view(np.uint8))
        s.close()


# ---- 6. ties and short lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_ties_go_to_the_lower_rank(ctx, oracle, metric):
    rng = np.random.default_rng(23)
    N = 600
    rows = rng.standard_normal((N, D)).astype(np.float32)
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(N, 1))).astype(np.float32)
    rows[100:109] = rows[500]  # ten equal rows: positions 100..108 and 500
    ids = np.arange(N, dtype=np.int64) * 3 + 50
    s = pa.Searcher(ctx, D, metric)
    s.add_rows(1, rows, ids)
    s.finalize()
    q = rows[500:501].copy()
    ref = Reference(oracle, q, rows, ids, metric)
    assert ref.pos[0, :10].tolist() == list(range(100, 109)) + [500]  # equal scores: the lower position first
    # equal rows have equal m at every step: they are picked in rank order wherever they are picked
    for lam in (1.0, 0.9, 0.5, 0.0):
        for k, pool in ((10, 128), (128, 128)):
            got = s.search_diverse(None, k, q, lam, pool=pool)
            check(got, ref.walk(0, k, lam, pool), 0, k)
            where = [int(np.nonzero(got[3][0] == r)[0][0]) for r in range(10) if (got[3][0] == r).any()]
            assert where == sorted(where) and where[0] == 0
    # lambda = 0: only redundancy counts, and a copy of a picked row (cosine 1 with it) is the last thing the walk wants
    got = s.search_diverse(None, 128, q, 0.0, pool=128)
    assert got[3][0, 0] == 0 and sorted(got[3][0, -9:].tolist()) == list(range(1, 10))
    s.close()


def test_short_lists_and_rows_without_a_score(ctx, oracle):
    """A list shorter than the pool ends inside it: every row is picked and the certificate holds.  A zero row has no cosine score
    and never appears under the cosine metric; under the dot metric its canonical score is 0 and pcv_searcher_search lists it, so
    it is in L here too (a pair with it counts as cosine 0)."""
    rng = np.random.default_rng(29)
    N = 100
    rows = rng.standard_normal((N, D)).astype(np.float32)
    ids = np.arange(N, dtype=np.int64) + 9
    q = rng.standard_normal((3, D)).astype(np.float32)
    zeroed = rows.copy()
    zeroed[[7, 60]] = 0.0
    for metric, data, n in (("cosine", rows, N), ("dot", rows, N), ("cosine", zeroed, N - 2), ("dot", zeroed, N)):
        s = pa.Searcher(ctx, D, metric)
        s.add_rows(1, data, ids)
        s.finalize()
        ref = Reference(oracle, q, data, ids, metric)
        for lam in (0.5, 0.0):
            got = s.search_diverse(None, 128, q, lam, pool=128)
            plain = s.search_vectors(None, 128, q)
            for b in range(3):
                check(got, ref.walk(b, 128, lam, 128), b, 128)
                assert int(got[4][b]) == n and int(got[5][b]) == n and bool(got[6][b])
                assert sorted(got[0][b, :n].tolist()) == sorted(plain[0][b, :n].tolist())  # the rows of L, each once
                assert np.isin(ids[[7, 60]], got[0][b]).all() == (n == N)
        s.close()


# ---- 7. the certificate --------------------------------------------------------------------------------------------------------
def test_certificate(ctx, planted):
    rows, ids, queries, ref = planted["cosine"]
    s = build_three_segments(ctx, "cosine", rows, ids, ("auto", "auto", "auto", 0))
    k, lam, pool = CERT["k"], CERT["lam"], CERT["pool"]
    got = s.search_diverse(None, k, queries, lam, pool=pool)
    for q in range(16):
        want = ref.walk(q, k, lam, pool)
        check(got, want, q, k)  # (out_exact equals the reference's flag)
        if got[6][q]:  # a 1 is a proof: the walk over ALL of L makes these picks
            full = ref.walk(q, k, lam, None)
            np.testing.assert_array_equal(got[3][q], full.ranks)
            np.testing.assert_array_equal(got[0][q], full.ids)
            np.testing.assert_array_equal(dr.bits64(got[2][q]), dr.bits64(full.marginal))
    assert got[6].any() and not got[6].all()
    # with the whole list in the pool the flag is case (a) or (b) as the reference has it, and the picks are the full walk's
    wide = s.search_diverse(None, k, queries[8:12], lam, pool=4096)
    for i, q in enumerate(range(8, 12)):
        full = ref.walk(q, k, lam, None)
        assert wide[6][i] and int(wide[5][i]) == rows.shape[0]
        np.testing.assert_array_equal(wide[3][i], full.ranks)
        np.testing.assert_array_equal(dr.bits64(wide[2][i]), dr.bits64(full.marginal))
    s.close()


# ---- 8. hidden, updated and removed items, a view, search by example -----------------------------------------------------------
def test_changes_views_and_like(ctx, oracle):
    metric = "cosine"
    rows, ids, anchors = planted_corpus(metric, seed=9)
    rng = np.random.default_rng(3)
    queries = planted_queries(metric, anchors, D, seed=3)[[0, 1, 2, 3, 8, 9, 10, 11]]  # four noisy anchors, four Gaussian rows
    N = rows.shape[0]
    K, LAM, POOL = 10, 0.5, 256
    s = build_three_segments(ctx, metric, rows, ids, ("auto", "auto", "auto", 0))

    def same_as_fresh(cur_rows, cur_ids, allowed=None, searcher=None):
        ref = Reference(oracle, queries, cur_rows, cur_ids, metric)
        got = (searcher or s).search_diverse(None, K, queries, LAM, pool=POOL)
        for q in range(len(queries)):
            check(got, ref.walk(q, K, LAM, POOL, allowed), q, K)
        return got

    base = same_as_fresh(rows, ids)
    assert (base[3][:4].max(axis=1) >= 60).all()  # the anchors' families were left behind
    # hidden rows are not in the list and come back
    hide = np.unique(np.concatenate([base[0][0, :3], base[0][5, :6]]))
    s.hide_items(hide)
    got = same_as_fresh(rows, ids, allowed=np.nonzero(~np.isin(ids, hide))[0])
    assert not np.isin(got[0], hide).any()
    s.unhide_items(hide)
    again = same_as_fresh(rows, ids)
    np.testing.assert_array_equal(again[0], base[0])
    # updated items: as a searcher built from the new rows
    at = [10, 500, 2500, 3000]
    new_rows = rows.copy()
    new_rows[at] = (anchors[0] + 0.01 * rng.standard_normal((4, D))).astype(np.float32)
    s.update_items(ids[at], new_rows[at])
    same_as_fresh(new_rows, ids)
    # a view: only its rows
    v = s.view(ids[::3])
    same_as_fresh(new_rows, ids, allowed=np.arange(0, N, 3), searcher=v)
    v.close()
    # search by example: the item itself first, then a diverse set of neighbours
    item = int(base[0][1, 0])
    row_of = int(np.nonzero(ids == item)[0][0])
    items = s.search_diverse_like_item(None, K, item, LAM, pool=POOL)
    ref1 = Reference(oracle, new_rows[row_of : row_of + 1], new_rows, ids, metric)
    want = ref1.walk(0, K, LAM, POOL)
    assert items[0].id == item and [it.id for it in items] == [int(x) for x in want.ids] and len(items) == K
    np.testing.assert_array_equal(bits32([it.score for it in items]), bits32(want.scores))
    with pytest.raises(KeyError):
        s.search_diverse_like_item(None, K, -12345, LAM)
    # removed items: as a searcher built without them
    gone = ids[np.r_[5:40, 1990:2020, N - 7 : N]]
    s.remove_items(gone)
    stay = ~np.isin(ids, gone)
    same_as_fresh(new_rows[stay], ids[stay])
    s.close()


# ---- 9. the refusals -----------------------------------------------------------------------------------------------------------
def test_unfinalized_searcher_gives_the_error_of_search(ctx):
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((40, 32)).astype(np.float32)
    s = pa.Searcher(ctx, 32, "cosine")
    s.add_rows(1, rows, np.arange(40))
    with pytest.raises(pa.PcvError) as plain:
        s.search_vectors(None, 5, rows[:1])
    with pytest.raises(pa.PcvError) as diverse:
        s.search_diverse(None, 5, rows[:1], 0.5)
    assert diverse.value.status == plain.value.status
    tail = "rows were added or cleared without pcv_searcher_finalize"
    assert str(plain.value).endswith(tail) and str(diverse.value).endswith("search_diverse: " + tail)
    s.finalize()
    ids, _scores, marginal, ranks, counts, examined, exact = s.search_diverse(None, 5, rows[:1], 1.0)
    assert counts[0] == 5 and ids[0, 0] == 0 and examined[0] == 40 and exact[0] and ranks[0].tolist() == [0, 1, 2, 3, 4]
    assert not np.isnan(marginal).any()
    s.close()


# ---- 10. the C++ mirror --------------------------------------------------------------------------------------------------------
def test_cpp_mirror_diverse_program():
    src = os.path.join(ROOT, "tests", "cpp", "diverse_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "diverse_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "diverse_mirror_test: ok" in r.stdout
