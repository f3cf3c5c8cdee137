"""GPU: boosted search (pcv_searcher_search_boosted), through the C ABI.  The reference of every check is tests/boost_ref.py:
oracle.topk over all rows gives the ranked list, the boost, the walk in steps of 128 and the certificate are Python written from the
definition, and a brute force over the whole list stands beside them.  Ids, values, ranks, counts, examined and exact are compared
for equality, scores by their bits against search_vectors, boosted scores by their bits against the model."""
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from boost_ref import NO_VALUE, Boost, BoostReference, bits32, bits64, check, default_pool
from perceive_amd.search import PCV_MAX_BOOST_POOL
from test_distinct_gpu import FORMS, build_three_segments, planted_corpus, planted_queries
from test_view_gpu import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384
I64 = np.iinfo(np.int64)
SPAN = 1 << 20


def value_of(ids, seed=3):
    """A seeded function of the id: even values in [-SPAN, SPAN), none (NO_VALUE) for about one id in eight."""
    with np.errstate(over="ignore"):
        h = (np.asarray(ids, dtype=np.int64).astype(np.uint64) + np.uint64(seed)) * np.uint64(0xD1B54A32D192ED03)
    h ^= h >> np.uint64(29)
    v = (2 * ((h >> np.uint64(8)) % np.uint64(SPAN))).astype(np.int64) - SPAN
    return np.where((h & np.uint64(7)) == 0, NO_VALUE, v)


def table_of(ids, seed=3):
    return {int(i): int(v) for i, v in zip(np.asarray(ids).tolist(), value_of(ids, seed).tolist()) if v != NO_VALUE}


def set_table(s, table):
    s.set_values(np.fromiter(table.keys(), dtype=np.int64, count=len(table)), np.fromiter(table.values(), dtype=np.int64, count=len(table)))


def rising(w):
    """recency-like: nothing for the oldest values, w for the newest, steeper towards the end"""
    return Boost([-SPAN, -SPAN // 2, 0, SPAN // 2, SPAN - 2], [0.0, w / 8, w / 4, w / 2, w], 0.0)


SMALL = rising(0.02)                                        # every query is certified inside one or two steps
FALLING = Boost([-SPAN // 2, 0, SPAN // 3], [0.3, -0.1, -0.4], 0.0)  # falling boosts, negative values, negative boosts
UNSET_ABOVE = Boost([0], [0.01], 0.05)                      # one knot: a constant, and b_max comes from the unset boost
ZERO = Boost([0], [0.0], 0.0)
KNOTS = {"small": SMALL, "falling": FALLING, "unset_above": UNSET_ABOVE}


def boosted(s, sources, k, queries, boost, pool=None):
    values, boosts, unset = boost.args()
    return s.search_boosted(sources, k, queries, values, boosts, unset, pool)


@pytest.fixture(scope="module")
def corpus(oracle):
    """the planted corpus of test_distinct_gpu.py per metric, its queries, the values of its ids and the ranked lists (computed once);
    `walks` remembers the model's walks: every screen form asks for the same ones"""
    out = {}
    for metric in ("cosine", "dot"):
        rows, ids, anchors = planted_corpus(metric)
        queries = planted_queries(metric, anchors, D)
        out[metric] = (rows, ids, queries, table_of(ids), BoostReference(oracle, queries, rows, ids, metric), {})
    return out


def plain_lists(s, queries, n):
    """the whole ranked list of every query from search_vectors: what out_scores and out_ranks are held against"""
    p_ids, p_scores, p_counts = s.search_vectors(None, n, queries)
    assert (p_counts == n).all()
    return p_ids, p_scores


def check_against_plain(got, plain, q):
    """the kept rows' ids and score bits are search_vectors' at their ranks"""
    ids, scores, _b, _v, ranks, counts, _e, _x = got
    n = int(counts[q])
    np.testing.assert_array_equal(ids[q, :n], plain[0][q, ranks[q, :n]])
    np.testing.assert_array_equal(bits32(scores[q, :n]), bits32(plain[1][q, ranks[q, :n]]))


# ---- 1. parity with the model ---------------------------------------------------------------------------------------------------
CASES = [(k, pool) for k in (1, 10, 128) for pool in sorted({k, 128, 129, 300, PCV_MAX_BOOST_POOL}) if pool >= k]
assert PCV_MAX_BOOST_POOL == 4096


def test_the_small_weights_are_certified_in_the_model(corpus):
    """(what test_parity relies on, from the reference alone)"""
    for metric in ("cosine", "dot"):
        _rows, _ids, _queries, table, ref, _walks = corpus[metric]
        for k, pool in ((1, 128), (10, 128), (10, 129), (10, 4096), (128, 4096)):
            ws = [ref.walk(q, k, pool, table, SMALL) for q in range(16)]
            print(metric, k, pool, [w.examined for w in ws])
            assert all(w.exact for w in ws)
            for q, w in enumerate(ws):  # ... and what the model certifies is the brute force's
                b = ref.brute(q, k, table, SMALL)
                assert w.ranks.tolist() == b.ranks.tolist() and bits64(w.boosted).tolist() == bits64(b.boosted).tolist()
        assert any(ref.walk(q, 128, 4096, table, SMALL).examined > 128 for q in range(16))  # more than one pass


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("form", list(FORMS))
def test_parity(ctx, corpus, form, metric):
    rows, ids, queries, table, ref, walks = corpus[metric]
    s = build_three_segments(ctx, metric, rows, ids, FORMS[form])
    set_table(s, table)
    plain = plain_lists(s, queries, rows.shape[0])
    n_exact = n_open = n_deep = 0
    for name, boost in KNOTS.items():
        for k, pool in CASES:
            got = boosted(s, None, k, queries, boost, pool)
            for q in range(16):
                key = (name, k, pool, q)
                if key not in walks:
                    walks[key] = ref.walk(q, k, pool, table, boost)
                want = walks[key]
                check(got, want, q, k)
                check_against_plain(got, plain, q)
                n_exact += want.exact
                n_open += not want.exact
                n_deep += want.examined > 128
                if got[7][q]:  # a 1 is a proof: the rows are those of the whole list
                    bkey = (name, k, q)
                    if bkey not in walks:
                        walks[bkey] = ref.brute(q, k, table, boost)
                    check(got, walks[bkey], q, k, rows_only=True)
    print(form, metric, "exact", n_exact, "not exact", n_open, "more than one pass", n_deep)
    assert n_exact > 100 and n_open > 100 and n_deep > 50
    # the default pool is search_where's rule
    got = boosted(s, None, 10, queries, SMALL)
    for q in range(16):
        check(got, walks[("small", 10, default_pool(10), q)], q, 10)
    s.close()


# ---- 2. a zero boost is the plain search ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_zero_boost(ctx, corpus, metric):
    rows, ids, queries, table, _ref, _walks = corpus[metric]
    s = build_three_segments(ctx, metric, rows, ids, FORMS["mfma_int8"])
    set_table(s, table)
    for k, pool in ((1, 1), (10, 10), (10, 128), (10, 4096), (128, 128), (128, 4096)):
        got = boosted(s, None, k, queries, ZERO, pool)
        p_ids, p_scores, p_counts = s.search_vectors(None, k, queries)
        np.testing.assert_array_equal(got[0], p_ids)
        np.testing.assert_array_equal(bits32(got[1]), bits32(p_scores))
        np.testing.assert_array_equal(got[3], value_of(p_ids))
        np.testing.assert_array_equal(got[4], np.tile(np.arange(k, dtype=np.int32), (16, 1)))
        np.testing.assert_array_equal(got[5], p_counts)
        assert got[7].all() and (got[6] == min(128, pool)).all()  # (|L| = the whole corpus: more than 128)
    # ... also where the list is shorter than a step
    got = boosted(s, [1], 10, queries, ZERO, 4096)
    assert got[7].all() and (got[6] == 128).all()
    short = pa.Searcher(ctx, D, metric)
    short.add_rows(1, rows[:50], ids[:50])
    short.finalize()
    got = boosted(short, None, 10, queries, ZERO, 4096)
    assert got[7].all() and (got[6] == 50).all() and (got[5] == 10).all()
    np.testing.assert_array_equal(got[0], short.search_vectors(None, 10, queries)[0])
    short.close()
    s.close()


# ---- 3. a tier is filtered search -----------------------------------------------------------------------------------------------
TIER_AT = 7 * SPAN // 8  # about one valued row in sixteen lies above it


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_a_tier_is_search_where(ctx, corpus, metric):
    rows, ids, queries, table, ref, _walks = corpus[metric]
    tier = Boost([TIER_AT, TIER_AT + 1], [0.0, 4.0], 0.0)
    k = 10
    model = [ref.walk(q, k, 4096, table, tier) for q in range(16)]
    for w in model:  # every query has its num_results boosted rows inside the prefix: the kept rows are all of the tier
        assert len(w.values) == k and (w.values > TIER_AT).all() and w.exact
    assert sum(w.examined > 128 for w in model) >= 4  # (some of them only in a later pass)
    s = build_three_segments(ctx, metric, rows, ids, FORMS["mfma_int8"])
    set_table(s, table)
    got = boosted(s, None, k, queries, tier, 4096)
    where = s.search_where(None, k, queries, TIER_AT + 1, int(I64.max), pool=4096)
    np.testing.assert_array_equal(got[0], where[0])
    np.testing.assert_array_equal(bits32(got[1]), bits32(where[1]))
    np.testing.assert_array_equal(got[3], where[2])
    np.testing.assert_array_equal(got[5], where[3])
    for q in range(16):
        check(got, model[q], q, k)
    s.close()


# ---- 4. ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_ties_go_to_the_lower_rank_across_passes(ctx, corpus, metric):
    rows, ids, queries, table, ref, _walks = corpus[metric]
    huge = Boost([0], [2.0 ** 60], 0.0)  # m = fl(rel + 2^60) = 2^60 for every valued row
    s = build_three_segments(ctx, metric, rows, ids, FORMS["mfma_int8"])
    set_table(s, table)
    plain = plain_lists(s, queries, 1024)
    for k, pool in ((128, 4096), (125, 300), (10, 4096)):
        got = boosted(s, None, k, queries, huge, pool)
        for q in range(16):
            want = ref.walk(q, k, pool, table, huge)
            check(got, want, q, k)
            assert (got[2][q] == 2.0 ** 60).all()
            valued = np.nonzero(value_of(plain[0][q]) != NO_VALUE)[0][:k]  # the valued rows in rank order
            np.testing.assert_array_equal(got[4][q], valued)
            if k == 128:  # a row kept in the first pass beat an equal m that came in a later one
                assert want.examined > 128 and got[4][q, 0] < 128 <= got[4][q, -1]
    s.close()


# ---- 5. a walk that ends at the pool uncertified ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_an_uncertified_walk(ctx, corpus, metric):
    rows, ids, all_queries, table, ref, _walks = corpus[metric]
    heavy, k = rising(3.0), 10
    qs = list(range(8, 16))  # the Gaussian queries: nothing stands out of their lists
    queries = all_queries[8:]
    model = [ref.walk(q, k, 128, table, heavy) for q in qs]
    assert not any(w.exact for w in model) and all(w.examined == 128 for w in model)
    s = build_three_segments(ctx, metric, rows, ids, FORMS["mfma_int8"])
    set_table(s, table)
    got = boosted(s, None, k, queries, heavy, 128)
    assert not got[7].any()
    differ = 0
    for i, q in enumerate(qs):
        shifted = [a[i : i + 1] for a in got]
        check(shifted, model[i], 0, k)
        differ += model[i].ranks.tolist() != ref.brute(q, k, table, heavy).ranks.tolist()
    assert differ >= 4  # (the flag is not idle: most of these answers are not those of the whole list)
    got = boosted(s, None, k, queries, heavy, 4096)
    assert got[7].all()
    for i, q in enumerate(qs):
        shifted = [a[i : i + 1] for a in got]
        check(shifted, ref.walk(q, k, 4096, table, heavy), 0, k)
        check(shifted, ref.brute(q, k, table, heavy), 0, k, rows_only=True)
    s.close()


# ---- 6. the edges of the walk -------------------------------------------------------------------------------------------------------
def test_edges_of_the_walk(ctx, oracle):
    rng = np.random.default_rng(129)
    n = [129, 5, 128, 300]  # sources 1 .. 4
    rows = rng.standard_normal((sum(n), D)).astype(np.float32)
    ids = (rng.permutation(sum(n)) * 3 + 50).astype(np.int64)
    queries = rng.standard_normal((4, D)).astype(np.float32)
    bounds = np.concatenate([[0], np.cumsum(n)])
    parts = [(src + 1, rows[bounds[src] : bounds[src + 1]], ids[bounds[src] : bounds[src + 1]]) for src in range(4)]
    s = build(ctx, D, "cosine", parts, screen="int8", kernel="mfma")
    table = table_of(ids)
    set_table(s, table)
    ref = BoostReference(oracle, queries, rows, ids, "cosine")
    heavy = rising(3.0)

    def run(sources, k, pool, boost=heavy):
        allowed = None if sources is None else np.concatenate([np.arange(bounds[x - 1], bounds[x]) for x in sources] + [np.zeros(0, np.int64)]).astype(np.int64)
        got = boosted(s, sources, k, queries, boost, pool)
        want = [ref.walk(q, k, pool, table, boost, allowed) for q in range(4)]
        for q in range(4):
            check(got, want[q], q, k)
        return got, want

    # a source of 129 rows: the second pass delivers one hit and the list ends
    got, want = run([1], 10, 4096)
    assert (got[6] == 129).all() and got[7].all()
    # pool 129: the second step asks for one entry and gets it — the list did not end, the pool did
    got, want = run(None, 10, 129)
    assert (got[6] == 129).all()
    got, want = run([1], 10, 129)  # ... |L| == pool exactly, and (b) fails (in the model): 0
    assert (got[6] == 129).all() and not any(w.exact for w in want)
    # a list shorter than num_results
    got, want = run([2], 10, 128)
    assert (got[5] == 5).all() and (got[6] == 5).all() and got[7].all() and (got[0][:, 5:] == -1).all()
    got, want = run([2], 128, 4096)
    assert (got[5] == 5).all()
    # a list of exactly `pool` entries, one step long
    got, want = run([3], 10, 128)
    assert (got[6] == 128).all() and not any(w.exact for w in want)
    got, want = run([3], 128, 128, SMALL)
    assert (got[5] == 128).all() and not any(w.exact for w in want)
    got, want = run([3], 10, 129)  # one entry more is asked for and none comes: the list ended
    assert (got[6] == 128).all() and got[7].all()
    # two sources, two steps and a bit
    got, want = run([1, 4], 10, 4096)
    assert (got[6] == 429).all() and got[7].all()
    got, want = run([3, 4, 2], 128, 300)
    # an empty selection: the blank answer, exact
    got = boosted(s, [], 10, queries, heavy, 128)
    assert (got[5] == 0).all() and (got[6] == 0).all() and got[7].all()
    assert (got[0] == -1).all() and np.isnan(got[1]).all() and np.isnan(got[2]).all() and (got[3] == NO_VALUE).all() and (got[4] == -1).all()
    s.close()


def test_seventy_queries_in_one_call(ctx, corpus, oracle):
    rows, ids, planted, table, _ref, _walks = corpus["cosine"]
    rng = np.random.default_rng(70)
    queries = np.concatenate([planted, rng.standard_normal((54, D)).astype(np.float32)])
    queries = queries[rng.permutation(70)]  # the queries that finish early stand among those that walk on
    s = build_three_segments(ctx, "cosine", rows, ids, FORMS["mfma_int8"])
    set_table(s, table)
    ref = BoostReference(oracle, queries, rows, ids, "cosine")
    boost, k = rising(0.2), 10
    model = [ref.walk(q, k, 4096, table, boost) for q in range(70)]
    first = sum(w.examined == 128 for w in model)
    print("finished in the first pass:", first, "examined:", sorted({w.examined for w in model}))
    assert first >= 10 and 70 - first >= 10 and all(w.exact for w in model)
    got = boosted(s, None, k, queries, boost, 4096)
    for q in range(70):  # (a finished query's rows did not change while the others walked on)
        check(got, model[q], q, k)
    for q in (0, 33, 69):  # ... as in a call of its own
        one = boosted(s, None, k, queries[q : q + 1], boost, 4096)
        for a, b in zip(got, one):
            np.testing.assert_array_equal(a[q : q + 1].view(np.uint8) if a.dtype.kind == "f" else a[q : q + 1], b.view(np.uint8) if b.dtype.kind == "f" else b)
    s.close()


# ---- 7. values and views ---------------------------------------------------------------------------------------------------------
def test_values_and_views(ctx, corpus):
    rows, ids, queries, table, ref, _walks = corpus["cosine"]
    s = build_three_segments(ctx, "cosine", rows, ids, FORMS["mfma_int8"])
    boost, k = rising(0.2), 10
    # an empty table: every row gets unset_boost, and the result is the plain top-k
    for unset in (0.0, 0.75, -2.0):
        b = Boost(boost.values, boost.boosts, unset)
        got = boosted(s, None, k, queries, b, 128)
        for q in range(16):
            check(got, ref.walk(q, k, 128, {}, b), q, k)
        np.testing.assert_array_equal(got[0], s.search_vectors(None, k, queries)[0])
        assert (got[3] == NO_VALUE).all() and (unset != 0.75 or got[7].all())  # (the unset boost is b_max: one step certifies)
    set_table(s, table)
    got = boosted(s, None, k, queries, boost, 512)
    for q in range(16):
        check(got, ref.walk(q, k, 512, table, boost), q, k)
    # values change between two calls: the best row of query 8 loses its value, the row at rank 100 becomes the newest item
    base = ref.walk(8, k, 512, table, boost)
    L, _sc = ref.ranked(8)
    moved = dict(table)
    top, far = int(base.ids[0]), int(ids[L[100]])
    moved.pop(top, None)
    moved[far] = SPAN - 2
    s.set_values([top, far], [NO_VALUE, SPAN - 2])
    got = boosted(s, None, k, queries, boost, 512)
    for q in range(16):
        check(got, ref.walk(q, k, 512, moved, boost), q, k)
    assert far in got[0][8] and ref.walk(8, k, 512, moved, boost).ids.tolist() != base.ids.tolist()
    # a hidden row never appears
    hidden = np.unique(got[0][:6, 0])
    s.hide_items(hidden)
    shown = np.nonzero(~np.isin(ids, hidden))[0]
    got = boosted(s, None, k, queries, boost, 512)
    for q in range(16):
        check(got, ref.walk(q, k, 512, moved, boost, shown), q, k)
    assert not np.isin(got[0], hidden).any()
    # an id-list view and a predicate view read the parent's table and walk their own rows
    half = ids[::2]
    v = s.view(half)
    in_view = np.nonzero(np.isin(ids, half) & ~np.isin(ids, hidden))[0]
    got = boosted(v, None, k, queries, boost, 512)
    for q in range(16):
        check(got, ref.walk(q, k, 512, moved, boost, in_view), q, k)
    w = s.view_where(0, int(I64.max), unset_passes=True)
    passing = np.array([moved.get(int(i), 0) >= 0 for i in ids.tolist()])
    in_w = np.nonzero(passing & ~np.isin(ids, hidden))[0]
    got = boosted(w, None, k, queries, boost, 512)
    for q in range(16):
        check(got, ref.walk(q, k, 512, moved, boost, in_w), q, k)
    # ... at call time
    newest = int(ids[in_view[-1]])
    s.set_values([newest], [SPAN - 2])
    moved[newest] = SPAN - 2
    got = boosted(v, None, k, queries, boost, 512)
    for q in range(16):
        check(got, ref.walk(q, k, 512, moved, boost, in_view), q, k)
    for view in (v, w):
        with pytest.raises(pa.PcvError) as err:
            view.set_values([1], [2])
        assert "the searcher is a view (read-only)" in str(err.value)
    v.close()
    w.close()
    # search by example: the item itself first under a zero boost
    s.unhide_items(hidden)
    item = int(ids[77])
    items = s.search_boosted_like_item(None, 5, item, *ZERO.args())
    assert items[0][0].id == item and len(items) == 5 and items[0][2] == moved.get(item, NO_VALUE)
    vec, _found, _members = s.like_queries([[item]])
    assert [it.id for it, _m, _v in items] == s.search_vectors(None, 5, vec)[0][0].tolist()
    with pytest.raises(KeyError):
        s.search_boosted_like_item(None, 5, -12345, *ZERO.args())
    one = s.search_boosted_vector(None, 3, queries[0], *boost.args())
    want = ref.walk(0, 3, 128, moved, boost)
    assert [it.id for it, _m, _v in one] == want.ids.tolist() and [m for _it, m, _v in one] == want.boosted.tolist()
    assert [v_ for _it, _m, v_ in one] == want.values.tolist()
    s.close()


def test_the_side_slot_carries_a_value(ctx, oracle):
    """the id INT64_MIN has no slot in the table: its value lives in the head block"""
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((200, D)).astype(np.float32)
    ids = np.arange(200, dtype=np.int64) + 1000
    ids[17] = I64.min
    queries = (rows[[17, 40]] + 0.3 * rng.standard_normal((2, D))).astype(np.float32)
    s = build(ctx, D, "cosine", [(1, rows, ids)], screen="int8", kernel="mfma")
    ref = BoostReference(oracle, queries, rows, ids, "cosine")
    boost = Boost([0, 100], [0.0, 0.5], -0.25)
    table = {}
    for change in ({int(I64.min): 100}, {1040: 50, 1041: 100}, {int(I64.min): 0}):
        table.update(change)
        s.set_values(list(change.keys()), list(change.values()))
        got = boosted(s, None, 5, queries, boost, 128)
        for q in range(2):
            check(got, ref.walk(q, 5, 128, table, boost), q, 5)
        assert got[0][0, 0] == I64.min and got[3][0, 0] == table[int(I64.min)]
    s.set_values([int(I64.min)], [NO_VALUE])
    del table[int(I64.min)]
    got = boosted(s, None, 5, queries, boost, 128)
    for q in range(2):
        check(got, ref.walk(q, 5, 128, table, boost), q, 5)
    s.close()


def test_unfinalized_searcher_gives_the_error_of_search(ctx):
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((40, 32)).astype(np.float32)
    s = pa.Searcher(ctx, 32, "cosine")
    s.add_rows(1, rows, np.arange(40))
    with pytest.raises(pa.PcvError) as plain:
        s.search_vectors(None, 5, rows[:1])
    with pytest.raises(pa.PcvError) as boost:
        boosted(s, None, 5, rows[:1], ZERO)
    assert boost.value.status == plain.value.status
    assert str(boost.value).endswith("search_boosted: rows were added or cleared without pcv_searcher_finalize")
    s.finalize()
    got = boosted(s, None, 5, rows[:1], ZERO)
    assert got[5][0] == 5 and got[7][0] and got[6][0] == 40
    s.close()


# ---- 8. the C++ mirror --------------------------------------------------------------------------------------------------------------
def hashed_rows(n, dim):
    """the rows of tests/cpp/boost_mirror_test.cpp"""
    i = np.arange(n, dtype=np.uint64)[:, None]
    j = np.arange(dim, dtype=np.uint64)[None, :]
    m = np.uint64(0xFFFFFFFF)
    h = (i * np.uint64(2654435761) + j * np.uint64(40503) + np.uint64(12345)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & m
    h ^= h >> np.uint64(13)
    return ((h >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0) - np.float32(0.5)).astype(np.float32)


def test_cpp_mirror_boost_program(ctx):
    src = os.path.join(ROOT, "tests", "cpp", "boost_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "boost_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "boost_mirror_test: ok" in r.stdout
    printed = [[int(x) for x in line.split()[1:]] for line in r.stdout.splitlines() if line.startswith("row ")]
    exact = [int(line.split()[1]) for line in r.stdout.splitlines() if line.startswith("exact ")]
    assert len(printed) == 10 and len(exact) == 1
    # the same searcher and the same call from Python
    n = 1500
    rows = hashed_rows(n, D)
    ids = np.arange(n, dtype=np.int64) + 9000
    odd = np.arange(n) % 2 == 1
    s = pa.Searcher(ctx, D, "cosine")
    s.add_rows(1, rows[~odd], ids[~odd])
    s.add_rows(2, rows[odd], ids[odd])
    s.finalize()
    has = np.arange(n) % 7 != 3
    s.set_values(ids[has], 10 * np.arange(n, dtype=np.int64)[has])
    got = s.search_boosted([1, 2], 10, rows[77:78], [0, 15000], [0.0, 0.05], 0.02, 128)
    assert got[5][0] == 10
    ours = [[int(got[0][0, j]), int(bits32(got[1][0, j : j + 1])[0]), int(bits64(got[2][0, j : j + 1])[0]), int(got[3][0, j]), int(got[4][0, j])] for j in range(10)]
    assert printed == ours and exact == [int(got[7][0])]
    s.close()
