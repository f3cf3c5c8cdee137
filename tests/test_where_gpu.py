"""GPU: item values and filtered search (pcv_searcher_set_values ... pcv_searcher_create_view_where), through the C ABI.  The
reference of every search check is tests/where_ref.py: oracle.topk over all rows gives the ranked list, a Python walk applies the
predicate to a dict id -> value.  Ids, values, counts, examined and more are compared for equality, scores by their bits; counts are
compared with numpy over the rows' ids; a predicate view with a searcher built fresh from the passing rows (test_view_gpu.py)."""
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from perceive_amd import _ffi
from test_distinct_gpu import FORMS, SPLIT, build_three_segments, planted_corpus, planted_queries
from test_view_gpu import allowed_parts, assert_same, build
from where_ref import NO_VALUE, OUTSIDE, UNSET_PASSES, WhereReference, check, default_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384
I64 = np.iinfo(np.int64)
EVERY = (I64.min + 1, I64.max)  # the interval every value lies in
SPAN = 1 << 20


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def value_of(ids, seed=3):
    """A seeded function of the id: EVEN values in [0, 2 * SPAN), none (NO_VALUE) for about one id in eight.  The interval ends the
    tests use are odd, so no value ties with one."""
    with np.errstate(over="ignore"):
        h = (np.asarray(ids, dtype=np.int64).astype(np.uint64) + np.uint64(seed)) * np.uint64(0xD1B54A32D192ED03)
    h ^= h >> np.uint64(29)
    v = (2 * ((h >> np.uint64(8)) % np.uint64(SPAN))).astype(np.int64)
    return np.where((h & np.uint64(7)) == 0, NO_VALUE, v)


def table_of(ids, seed=3):
    return {int(i): int(v) for i, v in zip(np.asarray(ids).tolist(), value_of(ids, seed).tolist()) if v != NO_VALUE}


def set_table(s, table):
    s.set_values(np.fromiter(table.keys(), dtype=np.int64, count=len(table)), np.fromiter(table.values(), dtype=np.int64, count=len(table)))


def flags_of(unset_passes, outside):
    return (UNSET_PASSES if unset_passes else 0) | (OUTSIDE if outside else 0)


def np_passes(ids, table, lo, hi, flags):
    """per row: does it pass?  (numpy over the rows' ids)"""
    ids = np.asarray(ids, dtype=np.int64).tolist()
    has = np.array([i in table for i in ids], dtype=bool)
    val = np.array([table.get(i, 0) for i in ids], dtype=np.int64)
    inside = (val >= lo) & (val <= hi)
    return np.where(has, inside != bool(flags & OUTSIDE), bool(flags & UNSET_PASSES))


@pytest.fixture(scope="module")
def corpus(oracle):
    """the planted corpus of test_distinct_gpu.py per metric, its queries, the values of its ids and the ranked lists (computed once)"""
    out = {}
    for metric in ("cosine", "dot"):
        rows, ids, anchors = planted_corpus(metric)
        queries = planted_queries(metric, anchors, D)
        out[metric] = (rows, ids, queries, table_of(ids), WhereReference(oracle, queries, rows, ids, metric))
    return out


# ---- 1. the table alone ------------------------------------------------------------------------------------------------------
def test_table_alone(ctx):
    s = pa.Searcher(ctx, 8, "cosine")  # no rows at all
    empty = {"ids": 0, "entries": 0, "slots": 0, "rehashes": 0, "last_set_ms": 0.0}
    assert s.value_stats() == empty
    assert (s.values_of([1, 2, I64.min]) == NO_VALUE).all()
    rng = np.random.default_rng(1)
    ids = np.unique(rng.integers(I64.min, I64.max, size=5200, dtype=np.int64))
    ids = rng.permutation(np.concatenate([ids[~np.isin(ids, [I64.min, -1, 0, 1, 2])][:4995], [I64.min, -1, 0, 1, 2]])).astype(np.int64)
    assert len(ids) == 5000 and len(np.unique(ids)) == 5000
    values = rng.integers(-(1 << 40), 1 << 40, size=5000, dtype=np.int64)
    values[ids == I64.min] = I64.max      # the largest value on the id that has no slot
    values[ids == -1] = I64.min + 1       # the smallest
    values[ids == 0] = 0
    values[ids == 1] = -1
    values[ids == 2] = I64.max
    assert (values < 0).sum() > 2000 and (values != NO_VALUE).all()
    for i0 in range(0, 5000, 700):
        s.set_values(ids[i0 : i0 + 700], values[i0 : i0 + 700])
        st = s.value_stats()
        n = min(i0 + 700, 5000)
        assert st["ids"] == n and st["entries"] == n
        assert st["slots"] >= 2 * n and st["slots"] & (st["slots"] - 1) == 0 and st["slots"] >= 1024
        assert st["last_set_ms"] > 0.0
    assert st["rehashes"] >= 2 and st["slots"] == 16384
    np.testing.assert_array_equal(s.values_of(ids), values)
    unknown = np.array([3, 4, I64.max, I64.min + 1], dtype=np.int64)
    assert not np.isin(unknown, ids).any() and (s.values_of(unknown) == NO_VALUE).all()
    assert s.values_of(np.zeros(0, np.int64)).shape == (0,)
    # duplicate ids in one batch: the last occurrence holds
    dup = ids[:200]
    batch_ids = np.concatenate([dup, dup, dup])
    batch_values = rng.integers(-(1 << 40), 1 << 40, size=600, dtype=np.int64)
    order = rng.permutation(600)
    batch_ids, batch_values = batch_ids[order], batch_values[order]
    last = {}
    for i, v in zip(batch_ids.tolist(), batch_values.tolist()):
        last[i] = v
    s.set_values(batch_ids, batch_values)
    np.testing.assert_array_equal(s.values_of(dup), np.array([last[i] for i in dup.tolist()], dtype=np.int64))
    np.testing.assert_array_equal(s.values_of(ids[200:]), values[200:])
    assert s.value_stats()["ids"] == 5000 and s.value_stats()["entries"] == 5000
    # ... also where the occurrences disagree on set / unset, and for new ids
    fresh = np.array([3, 4, 5], dtype=np.int64)
    s.set_values(np.array([3, 4, 3, 4, 3, 5, 5], dtype=np.int64), np.array([5, NO_VALUE, NO_VALUE, -6, -7, 8, NO_VALUE], dtype=np.int64))
    np.testing.assert_array_equal(s.values_of(fresh), [-7, -6, NO_VALUE])
    assert s.value_stats()["ids"] == 5002 and s.value_stats()["entries"] == 5003
    # unsetting: the entry stays, the id has no value; the side slot too
    gone = np.concatenate([ids[1000:1100][ids[1000:1100] != I64.min], [I64.min]]).astype(np.int64)
    s.set_values(gone, np.full(len(gone), NO_VALUE, dtype=np.int64))
    st = s.value_stats()
    assert st["ids"] == 5002 - len(gone) and st["entries"] == 5003
    assert (s.values_of(gone) == NO_VALUE).all()
    s.set_values(gone, np.full(len(gone), NO_VALUE, dtype=np.int64))  # again: nothing to count
    assert s.value_stats()["ids"] == 5002 - len(gone)
    # ... then set again
    s.set_values(gone[:50], -np.arange(50, dtype=np.int64))  # (0 and negative values are values)
    s.set_values(gone[-1:], np.array([I64.min + 1], dtype=np.int64))
    st = s.value_stats()
    assert st["ids"] == 5002 - len(gone) + 51 and st["entries"] == 5003
    np.testing.assert_array_equal(s.values_of(gone[:50]), -np.arange(50))
    assert s.values_of([I64.min])[0] == I64.min + 1
    # a refused batch changes nothing
    before = s.values_of(ids)
    with pytest.raises(pa.PcvError):
        _ffi.check(_ffi.lib().pcv_searcher_set_values(s._handle, _ffi.i64p(ids[:5].copy()), None, 5))
    with pytest.raises(ValueError):
        s.set_values([1, 2], [5])
    np.testing.assert_array_equal(s.values_of(ids), before)
    assert s.value_stats()["entries"] == 5003
    # groups and values set on the same ids read back independently
    assert s.group_stats()["entries"] == 0 and (s.groups_of(ids[:100]) == -1).all()
    groups = rng.integers(0, 1 << 40, size=300, dtype=np.int64)
    s.set_groups(ids[:300], groups)
    np.testing.assert_array_equal(s.groups_of(ids[:300]), groups)
    np.testing.assert_array_equal(s.values_of(ids), before)
    s.set_values(ids[:300], groups + 1)
    np.testing.assert_array_equal(s.groups_of(ids[:300]), groups)
    np.testing.assert_array_equal(s.values_of(ids[:300]), groups + 1)
    s.set_groups(ids[:10], np.full(10, -1, dtype=np.int64))  # (-1 ungroups and is an ordinary value)
    s.set_values(ids[:10], np.full(10, -1, dtype=np.int64))
    assert (s.groups_of(ids[:10]) == -1).all() and s.group_stats()["ids"] == 290
    assert (s.values_of(ids[:10]) == -1).all() and s.value_stats()["ids"] == 5002 - len(gone) + 51
    # clear: as created, and usable; the groups stay
    s.clear_values()
    assert s.value_stats() == empty
    assert (s.values_of(ids[:100]) == NO_VALUE).all() and s.values_of([I64.min])[0] == NO_VALUE
    assert s.group_stats()["ids"] == 290
    s.set_values(ids[:10], values[:10])
    st = s.value_stats()
    assert (st["ids"], st["entries"], st["slots"], st["rehashes"]) == (10, 10, 1024, 0)
    np.testing.assert_array_equal(s.values_of(ids[:12]), np.concatenate([values[:10], [NO_VALUE, NO_VALUE]]))
    s.close()


# ---- 2. count_where against numpy --------------------------------------------------------------------------------------------
COUNT_SOURCE = 9  # the implicit-id source


def count_cases(table):
    present = sorted(table.values())
    one = present[len(present) // 3]  # a value that occurs
    return [
        EVERY,
        (SPAN + 1, SPAN - 1),         # lo > hi: the empty interval
        (5, -5),
        (one, one),
        (I64.min + 1, SPAN - 1),      # one-sided, with the extremes
        (SPAN + 1, I64.max),
        (I64.min, I64.max),           # (lo == PCV_NO_VALUE is a bound like any other: no value equals it)
        (SPAN // 8 + 1, SPAN // 4 - 1),
    ]


@pytest.mark.parametrize("n_implicit", [1, 1023, 1025, 2049])
def test_count_where(ctx, corpus, n_implicit):
    rows, ids, _queries, _table, _ref = corpus["cosine"]
    s = build_three_segments(ctx, "cosine", rows, ids, FORMS["mfma_int8"])
    rng = np.random.default_rng(n_implicit)
    extra = rng.standard_normal((n_implicit, D)).astype(np.float32)
    s.add_rows(COUNT_SOURCE, extra)  # ids 0 .. n_implicit - 1, made on the device
    s.finalize()
    _r, extra_ids = s.get_rows(np.arange(len(ids), len(ids) + n_implicit))
    np.testing.assert_array_equal(extra_ids, np.arange(n_implicit))
    all_ids = np.concatenate([ids, extra_ids])
    src_of = np.concatenate([np.full(SPLIT[1], 1), np.full(len(ids) - SPLIT[1], 2), np.full(n_implicit, COUNT_SOURCE)])
    table = table_of(all_ids)
    # an empty table: nothing has a value
    for unset in (False, True):
        assert s.count_where(None, *EVERY, unset_passes=unset) == ((len(all_ids),) * 2 if unset else (0, 0))
        assert s.count_where(None, *EVERY, unset_passes=unset, outside=True) == ((len(all_ids),) * 2 if unset else (0, 0))
    set_table(s, table)
    hidden = np.concatenate([ids[5:60], ids[2500:2520], extra_ids[-3:]])
    for hide in (False, True):
        if hide:
            s.hide_items(hidden)
        live = ~np.isin(all_ids, hidden) if hide else np.ones(len(all_ids), dtype=bool)
        for lo, hi in count_cases(table):
            for unset in (False, True):
                for outside in (False, True):
                    ok = np_passes(all_ids, table, lo, hi, flags_of(unset, outside))
                    for sources, sel in ((None, np.ones(len(all_ids), dtype=bool)), ([2], src_of == 2), ([COUNT_SOURCE, 1], src_of != 2),
                                         ([COUNT_SOURCE], src_of == COUNT_SOURCE), ([], np.zeros(len(all_ids), dtype=bool))):
                        got = s.count_where(sources, lo, hi, unset_passes=unset, outside=outside)
                        want = (int((ok & sel).sum()), int((ok & sel & live).sum()))
                        print(n_implicit, hide, (lo, hi), unset, outside, sources, got, want)
                        assert got == want
    assert s.count_where(None, *EVERY) == (len(table_rows(all_ids, table)), len(table_rows(all_ids[~np.isin(all_ids, hidden)], table)))
    s.close()


def table_rows(ids, table):
    return [i for i in np.asarray(ids).tolist() if i in table]


def test_count_where_rows_without_an_id_column_and_a_view(ctx):
    """synthetic rows have no id column (id = id0 + row, made in the kernel); a view counts its own rows"""
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(4, 3001, 0xC0FFEE, first_row=100_000, normalize=True)  # implicit ids 100000 .. 103000
    s.finalize()
    ids = np.arange(100_000, 103_001)
    table = table_of(ids)
    set_table(s, table)
    for lo, hi in ((1, SPAN - 1), EVERY, (7, 3)):
        for unset in (False, True):
            for outside in (False, True):
                ok = np_passes(ids, table, lo, hi, flags_of(unset, outside))
                assert s.count_where(None, lo, hi, unset_passes=unset, outside=outside) == (int(ok.sum()),) * 2
    low = np_passes(ids, table, 1, SPAN - 1, 0)
    v = s.view(ids[::3])
    assert v.count_where(None, 1, SPAN - 1) == (int(low[::3].sum()),) * 2
    assert v.count_where(None, 1, SPAN - 1, unset_passes=True, outside=True) == (int((~low)[::3].sum()),) * 2
    assert v.count_where([5], 1, SPAN - 1) == (0, 0)
    v.close()
    s.close()


# ---- 3. search_where against the reference -----------------------------------------------------------------------------------
HALF = (-1, SPAN - 1)            # about half of the rows that have a value
SIXTEENTH = (-1, SPAN // 8 - 1)  # about one in sixteen


def test_the_selective_predicate_needs_more_than_one_pass(corpus):
    """(what the cases below rely on, from the reference alone)"""
    for metric in ("cosine", "dot"):
        _rows, _ids, _queries, table, ref = corpus[metric]
        deep = sum(1 for q in range(16) if ref.walk(q, 10, 1024, table, *SIXTEENTH)[3] > 128)
        print(metric, "queries that examine more than one pass:", deep)
        assert deep >= 4


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("form", list(FORMS))
def test_search_where(ctx, corpus, form, metric):
    rows, ids, queries, table, ref = corpus[metric]
    s = build_three_segments(ctx, metric, rows, ids, FORMS[form])
    set_table(s, table)
    assert s.value_stats()["ids"] == len(table)
    # a predicate everything passes: the plain search, bit for bit
    for k in (1, 10, 128):
        got = s.search_where(None, k, queries, *EVERY, unset_passes=True)
        p_ids, p_scores, p_counts = s.search_vectors(None, k, queries)
        np.testing.assert_array_equal(got[0], p_ids)
        np.testing.assert_array_equal(bits(got[1]), bits(p_scores))
        np.testing.assert_array_equal(got[2], value_of(p_ids))
        np.testing.assert_array_equal(got[3], p_counts)
        assert (got[4] == k).all() and not got[5].any()
        for q in range(16):
            check(got, ref.walk(q, k, default_pool(k), table, *EVERY, UNSET_PASSES), q, k)
    # about one row in two
    for B in (1, 16):
        for k in (1, 10, 128):
            for flags in (0, UNSET_PASSES, OUTSIDE, OUTSIDE | UNSET_PASSES):
                got = s.search_where(None, k, queries[:B], *HALF, unset_passes=bool(flags & UNSET_PASSES), outside=bool(flags & OUTSIDE))
                for q in range(B):
                    check(got, ref.walk(q, k, default_pool(k), table, *HALF, flags), q, k)
    # about one in sixteen: more than one pass (test_the_selective_predicate_needs_more_than_one_pass)
    got = s.search_where(None, 10, queries, *SIXTEENTH, pool=1024)
    for q in range(16):
        check(got, ref.walk(q, 10, 1024, table, *SIXTEENTH), q, 10)
    assert (got[4] > 128).sum() >= 4 and (got[3] == 10).all()
    got = s.search_where(None, 10, queries, *SIXTEENTH, pool=130)  # the pool ends inside the second pass
    for q in range(16):
        check(got, ref.walk(q, 10, 130, table, *SIXTEENTH), q, 10)
    assert got[5].any()
    # nothing passes: the walk runs to the end of the pool, and the list has more
    for lo, hi, pool in ((SPAN + 1, SPAN - 1, 128), (5, -5, 300)):
        got = s.search_where(None, 10, queries, lo, hi, pool=pool)
        for q in range(16):
            check(got, ref.walk(q, 10, pool, table, lo, hi), q, 10)
        assert (got[3] == 0).all() and (got[4] == min(pool, rows.shape[0])).all() and got[5].all()
    # a source filter: only the rows of source 2 — a list shorter than the pool ends without `more`
    allowed = np.arange(SPLIT[1], rows.shape[0])
    got = s.search_where([2], 10, queries, *SIXTEENTH, pool=200)
    for q in range(16):
        check(got, ref.walk(q, 10, 200, table, *SIXTEENTH, 0, allowed), q, 10)
    got = s.search_where([2], 10, queries[:4], 5, -5, pool=4096)
    assert (got[4] == len(allowed)).all() and not got[5].any() and (got[3] == 0).all()
    empty = s.search_where([], 10, queries[:3], *HALF)  # an empty filter matches nothing
    assert (empty[3] == 0).all() and (empty[0] == -1).all() and (empty[2] == NO_VALUE).all() and (empty[4] == 0).all() and not empty[5].any()
    s.close()


def test_search_where_without_a_table(ctx, corpus):
    rows, ids, queries, _table, ref = corpus["cosine"]
    s = build_three_segments(ctx, "cosine", rows, ids, FORMS["mfma_int8"])
    got = s.search_where(None, 10, queries, *EVERY)  # nothing has a value
    assert (got[3] == 0).all() and (got[4] == 128).all() and got[5].all()
    got = s.search_where(None, 10, queries, *EVERY, unset_passes=True)
    for q in range(16):
        check(got, ref.walk(q, 10, 128, {}, *EVERY, UNSET_PASSES), q, 10)
    assert (got[2] == NO_VALUE).all()
    s.close()


def test_seventy_queries_in_one_call(ctx, corpus, oracle):
    rows, ids, _queries, table, _ref = corpus["cosine"]
    rng = np.random.default_rng(70)
    queries = rng.standard_normal((70, D)).astype(np.float32)
    s = build_three_segments(ctx, "cosine", rows, ids, FORMS["mfma_int8"])
    set_table(s, table)
    ref = WhereReference(oracle, queries, rows, ids, "cosine", depth=1100)
    got = s.search_where(None, 10, queries, *SIXTEENTH, pool=1024)
    for q in range(70):
        check(got, ref.walk(q, 10, 1024, table, *SIXTEENTH), q, 10)
    assert (got[4] > 128).sum() >= 10
    for q in (0, 33, 69):  # ... as in a call of its own
        one = s.search_where(None, 10, queries[q : q + 1], *SIXTEENTH, pool=1024)
        for a, b in zip(got, one):
            np.testing.assert_array_equal(bits(a[q : q + 1]) if a.dtype == np.float32 else a[q : q + 1], bits(b) if b.dtype == np.float32 else b)
    s.close()


def test_search_where_on_a_view_with_hidden_items_and_by_example(ctx, corpus):
    rows, ids, queries, table, ref = corpus["cosine"]
    s = build_three_segments(ctx, "cosine", rows, ids, FORMS["mfma_int8"])
    set_table(s, table)
    base = s.search_where(None, 10, queries, *HALF)
    # hidden items: the best passing item of some queries goes, the next passing one takes its place
    best = np.unique(base[0][:6, 0])
    s.hide_items(best)
    shown = np.nonzero(~np.isin(ids, best))[0]
    got = s.search_where(None, 10, queries, *HALF)
    for q in range(16):
        check(got, ref.walk(q, 10, 128, table, *HALF, 0, shown), q, 10)
    assert not np.isin(got[0], best).any()
    # a view over half of the ids reads the parent's values, at call time
    half = ids[::2]
    v = s.view(half)
    in_view = np.nonzero(np.isin(ids, half) & ~np.isin(ids, best))[0]
    for flags in (0, OUTSIDE | UNSET_PASSES):
        got = v.search_where(None, 10, queries, *SIXTEENTH, unset_passes=bool(flags & UNSET_PASSES), outside=bool(flags & OUTSIDE), pool=512)
        for q in range(16):
            check(got, ref.walk(q, 10, 512, table, *SIXTEENTH, flags, in_view), q, 10)
    np.testing.assert_array_equal(v.values_of(ids[:50]), s.values_of(ids[:50]))
    assert v.value_stats() == s.value_stats()
    for change in (lambda: v.set_values([1], [2]), lambda: v.clear_values()):
        with pytest.raises(pa.PcvError) as err:
            change()
        assert "the searcher is a view (read-only)" in str(err.value)
    # ... at call time: the best row of query 0 outside the interval moves into it between two searches of the view
    moved = dict(table)
    first = int(got[0][0, 0])
    s.set_values([first], [SPAN // 16])
    moved[first] = SPAN // 16
    got = v.search_where(None, 10, queries, *SIXTEENTH, pool=512)
    for q in range(16):
        check(got, ref.walk(q, 10, 512, moved, *SIXTEENTH, 0, in_view), q, 10)
    assert first in got[0][0]
    assert v.view_stats()["refreshes"] == 0  # (an id-list view never looks at the values' generation)
    v.close()
    # search by example: the item itself first, if it passes
    s.unhide_items(best)
    item = int(base[0][2, 0])
    items = s.search_where_like_item(None, 5, item, *HALF)
    assert items[0][0].id == item and items[0][1] == moved[item] and len(items) == 5
    assert all(HALF[0] <= val <= HALF[1] for _it, val in items)
    with pytest.raises(KeyError):
        s.search_where_like_item(None, 5, -12345, *HALF)
    one = s.search_where_vector(None, 3, queries[0], *HALF)
    w = ref.walk(0, 3, 128, moved, *HALF)
    assert [it.id for it, _v in one] == w[0].tolist() and [val for _it, val in one] == w[2].tolist()
    s.close()


def test_unfinalized_searcher_gives_the_error_of_search(ctx):
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((40, 32)).astype(np.float32)
    s = pa.Searcher(ctx, 32, "cosine")
    s.add_rows(1, rows, np.arange(40))
    s.set_values(np.arange(40), np.arange(40))  # (the table does not wait for finalize)
    with pytest.raises(pa.PcvError) as plain:
        s.search_vectors(None, 5, rows[:1])
    with pytest.raises(pa.PcvError) as where:
        s.search_where(None, 5, rows[:1], 0, 100)
    with pytest.raises(pa.PcvError) as count:
        s.count_where(None, 0, 100)
    assert where.value.status == plain.value.status == count.value.status
    tail = "rows were added or cleared without pcv_searcher_finalize"
    assert str(where.value).endswith("search_where: " + tail) and str(count.value).endswith("count_where: " + tail)
    s.finalize()
    ids, _scores, values, counts, examined, more = s.search_where(None, 5, rows[:1], 10, 100)
    assert counts[0] == 5 and (values[0] >= 10).all() and not more[0] and examined[0] >= 5
    assert s.count_where(None, 10, 100) == (30, 30)
    s.close()


# ---- 4. predicate views --------------------------------------------------------------------------------------------------------
def view_parts(rows, ids):
    a, b = SPLIT
    return [(1, rows[:b], ids[:b]), (2, rows[b:], ids[b:])]


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_view_where_is_the_fresh_searcher(ctx, corpus, metric):
    rows, ids, queries, table, _ref = corpus[metric]
    rng = np.random.default_rng(4)
    s = build_three_segments(ctx, metric, rows, ids, FORMS["mfma_int8"])
    s.add_synthetic(4, 2500, 0xC0FFEE, first_row=100_000, normalize=True)  # rows without an id column: ids 100000 .. 102499
    own = rng.standard_normal((1500, D)).astype(np.float32)
    s.add_rows(COUNT_SOURCE, own)  # ids 0 .. 1499, made on the device
    s.finalize()
    syn, syn_ids = s.get_rows(np.arange(len(ids), len(ids) + 2500))
    np.testing.assert_array_equal(syn_ids, np.arange(100_000, 102_500))
    parts = view_parts(rows, ids) + [(4, syn, syn_ids), (COUNT_SOURCE, own, np.arange(1500, dtype=np.int64))]
    all_ids = np.concatenate([i for _s, _r, i in parts])
    table = table_of(all_ids)
    set_table(s, table)
    q = np.concatenate([queries, syn[::500], own[::400]])
    for (lo, hi), unset, outside in ((SIXTEENTH, False, False), (HALF, True, False), (HALF, False, True), ((SPAN // 4 + 1, SPAN // 4 + 4001), False, False)):
        ok = np_passes(all_ids, table, lo, hi, flags_of(unset, outside))
        allow = np.unique(all_ids[ok])
        sub = allowed_parts(parts, allow)
        v = s.view_where(lo, hi, unset_passes=unset, outside=outside)
        f = build(ctx, D, metric, sub, screen="int8", kernel="mfma")
        w = s.view(allow)
        st = v.view_stats()
        print(metric, (lo, hi), unset, outside, st, int(ok.sum()))
        assert st["rows"] == int(ok.sum()) == v.num_rows == f.num_rows and st["ids"] == 0 and st["refreshes"] == 0 and st["build_ms"] > 0
        assert v.source_ids == f.source_ids == w.source_ids
        assert s.count_where(None, lo, hi, unset_passes=unset, outside=outside)[0] == st["rows"]
        for k in (10, 200):
            got = v.search_vectors(None, k, q)
            assert_same(got, f.search_vectors(None, k, q))
            assert_same(got, w.search_vectors(None, k, q))
        assert_same(v.search_vectors([4, COUNT_SOURCE], 10, q), f.search_vectors([4, COUNT_SOURCE], 10, q))
        for x in (v, f, w):
            x.close()
    # nothing passes: an empty view
    e = s.view_where(5, -5)
    assert e.num_rows == 0 and e.source_ids == [] and e.view_stats()["rows"] == 0
    e_ids, e_sc, e_cnt = e.search_vectors(None, 10, q)
    assert (e_cnt == 0).all() and (e_ids == -1).all() and np.isnan(e_sc).all()
    with pytest.raises(pa.PcvError):
        e.view_where(0, 10)  # views of views stay refused
    e.close()
    s.close()


def test_view_where_staleness(ctx, corpus):
    rows, ids, queries, table, _ref = corpus["cosine"]
    parts = view_parts(rows, ids)
    s = build_three_segments(ctx, "cosine", rows, ids, FORMS["mfma_int8"])
    set_table(s, table)
    lo, hi = SIXTEENTH
    v = s.view_where(lo, hi)
    listed = s.view(ids[::5])  # an id-list view alive beside it
    state = {"table": dict(table), "parts": parts, "hidden": [], "flags": 0}

    def expect(view=v, interval=(lo, hi)):
        all_ids = np.concatenate([i for _s, _r, i in state["parts"]])
        ok = np_passes(all_ids, state["table"], interval[0], interval[1], state["flags"])
        f = build(ctx, D, "cosine", allowed_parts(state["parts"], np.unique(all_ids[ok])), screen="int8", kernel="mfma")
        if len(state["hidden"]):
            f.hide_items(state["hidden"])
        for k in (10, 129):
            assert_same(view.search_vectors(None, k, queries), f.search_vectors(None, k, queries))
        f.close()
        return int(ok.sum())

    n0 = expect()
    assert v.view_stats()["refreshes"] == 0 and listed.view_stats()["refreshes"] == 0
    # part 1: one id's value crosses the interval end — into the interval, then out of it
    outside_id = next(int(i) for i in ids.tolist() if i in table and table[int(i)] > hi and (ids == i).sum() == 1)
    s.set_values([outside_id], [hi - 1])
    state["table"][outside_id] = hi - 1
    assert expect() == n0 + 1
    st = v.view_stats()
    assert st["refreshes"] == 1 and st["rows"] == n0 + 1 and st["ids"] == 0
    assert outside_id in v.search_vectors(None, 1, rows[ids == outside_id])[0]
    s.set_values([outside_id], [hi + 1])
    state["table"][outside_id] = hi + 1
    assert expect() == n0
    assert v.view_stats()["refreshes"] == 2
    listed.search_vectors(None, 10, queries)
    assert listed.view_stats()["refreshes"] == 0  # set_values is nothing to an id-list view
    s.set_values([], [])  # (an empty batch changes nothing)
    assert v.view_stats()["refreshes"] == 2
    # part 2: hide, update and remove refresh it, as they refresh id-list views
    in_view = np.array([i for i in ids.tolist() if lo <= state["table"].get(int(i), hi + 1) <= hi], dtype=np.int64)
    hid = int(in_view[0])
    s.hide_items([hid])
    state["hidden"] = [hid]
    expect()
    assert v.view_stats()["refreshes"] == 3 and listed.view_stats()["refreshes"] == 1
    upd = int(in_view[1])
    vec = (3.0 * queries[0]).astype(np.float32)
    s.update_items([upd], vec[None])
    state["parts"] = [(src, r.copy(), i) for src, r, i in parts]
    for _s, r, i in state["parts"]:
        r[i == upd] = vec
    expect()
    assert v.view_stats()["refreshes"] == 4 and v.search_vectors(None, 1, queries[:1])[0][0, 0] == upd
    gone = in_view[2:5]
    gone = gone[[(ids == g).sum() == 1 for g in gone]]
    s.remove_items(gone)
    state["parts"] = [(src, r[~np.isin(i, gone)], i[~np.isin(i, gone)]) for src, r, i in state["parts"]]
    expect()
    st = v.view_stats()
    assert st["refreshes"] == 5 and st["rows"] == n0 - len(gone)
    np.testing.assert_array_equal(s.values_of(gone), [state["table"][int(g)] for g in gone])  # (the values outlive the rows)
    # clear_values empties it — or fills it under UNSET_PASSES
    u = s.view_where(lo, hi, unset_passes=True)
    s.clear_values()
    state["table"] = {}
    assert v.view_stats()["rows"] == 0 and v.view_stats()["refreshes"] == 6
    ids_e, _sc, cnt_e = v.search_vectors(None, 10, queries)
    assert (cnt_e == 0).all() and (ids_e == -1).all()
    state["flags"] = UNSET_PASSES
    assert expect(view=u) == sum(len(i) for _s, _r, i in state["parts"]) == u.view_stats()["rows"]
    assert u.view_stats()["refreshes"] == 1
    assert listed.view_stats()["refreshes"] == 2  # (one copy for the update and the removal together; none for clear_values)
    # the parent cannot go while the view lives
    assert _ffi.lib().pcv_searcher_destroy(s._handle) == 1
    assert "view(s) of this searcher are alive" in _ffi.lib().pcv_last_error().decode()
    for x in (u, v, listed):
        x.close()
    s.close()


# ---- 5. the C++ mirror -------------------------------------------------------------------------------------------------------
def test_cpp_mirror_where_program():
    src = os.path.join(ROOT, "tests", "cpp", "where_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "where_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "where_mirror_test: ok" in r.stdout
