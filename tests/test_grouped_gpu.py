"""GPU: the group table and grouped results (pcv_searcher_set_groups ... pcv_searcher_search_grouped), through the C ABI.  The
reference of every search check is tests/grouped_ref.py: oracle.topk over all rows gives the ranked list, a dict walk collapses it.
Ids, groups, counts, collapsed, examined and more are compared for equality, scores by their bits — against the reference and
against search_vectors on the same searcher."""
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from grouped_ref import GroupedReference, check, default_pool
from test_distinct_gpu import FORMS, build_three_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384
I64 = np.iinfo(np.int64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def id_hash(ids, mask):
    """corpus.h: the upper half of id * 0x9E3779B97F4A7C15 (mod 2^64), masked"""
    with np.errstate(over="ignore"):
        return ((np.asarray(ids, dtype=np.int64).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)).astype(np.int64) & mask


def scores_match_plain_search(s, got, queries, sources=None):
    """every kept row carries the score search_vectors reports for it (same searcher, same bits)"""
    ids, scores, _groups, counts, _collapsed, examined, _more = got
    depth = int(examined.max())
    if depth == 0:
        return
    for q in range(len(counts)):
        p_ids, p_scores, p_counts = s.search_vectors(sources, int(examined[q]), queries[q : q + 1])
        at = 0
        for j in range(int(counts[q])):  # the kept rows are a subsequence of the plain list
            while not (p_ids[0, at] == ids[q, j] and bits(p_scores[0, at]) == bits(scores[q, j])):
                at += 1
                assert at < int(p_counts[0]), (q, j)
            at += 1


# ---- 1. the table alone ------------------------------------------------------------------------------------------------------
def test_table_alone(ctx):
    s = pa.Searcher(ctx, 8, "cosine")  # no rows at all
    assert s.group_stats() == {"ids": 0, "entries": 0, "slots": 0, "rehashes": 0, "last_set_ms": 0.0}
    assert (s.groups_of([1, 2, I64.min]) == -1).all()
    rng = np.random.default_rng(1)
    ids = np.unique(rng.integers(I64.min, I64.max, size=5200, dtype=np.int64))[:4995]
    ids = rng.permutation(np.concatenate([ids[~np.isin(ids, [I64.min, -1, 0, 1, 2])][:4995], [I64.min, -1, 0, 1, 2]])).astype(np.int64)
    assert len(ids) == 5000 and len(np.unique(ids)) == 5000
    groups = rng.integers(0, 1 << 40, size=5000, dtype=np.int64)
    groups[ids == I64.min] = I64.max  # the largest key on the id that has no slot
    groups[ids == -1] = 0
    groups[ids == 0] = I64.max
    for i0 in range(0, 5000, 700):
        s.set_groups(ids[i0 : i0 + 700], groups[i0 : i0 + 700])
        st = s.group_stats()
        n = min(i0 + 700, 5000)
        assert st["ids"] == n and st["entries"] == n
        assert st["slots"] >= 2 * n and st["slots"] & (st["slots"] - 1) == 0 and st["slots"] >= 1024
        assert st["last_set_ms"] > 0.0
    assert st["rehashes"] >= 2 and st["slots"] == 16384
    np.testing.assert_array_equal(s.groups_of(ids), groups)
    unknown = np.array([3, 4, I64.max, I64.min + 1], dtype=np.int64)
    assert not np.isin(unknown, ids).any() and (s.groups_of(unknown) == -1).all()
    assert s.groups_of(np.zeros(0, np.int64)).shape == (0,)
    # duplicate ids in one batch: the last occurrence holds
    dup = ids[:200]
    batch_ids = np.concatenate([dup, dup, dup])
    batch_groups = rng.integers(0, 1 << 40, size=600, dtype=np.int64)
    order = rng.permutation(600)
    batch_ids, batch_groups = batch_ids[order], batch_groups[order]
    last = {}
    for i, g in zip(batch_ids.tolist(), batch_groups.tolist()):
        last[i] = g
    assert sum(1 for i in dup.tolist() if last[i] != groups[ids == i][0]) == 200  # (every id changes its group)
    s.set_groups(batch_ids, batch_groups)
    np.testing.assert_array_equal(s.groups_of(dup), np.array([last[i] for i in dup.tolist()], dtype=np.int64))
    np.testing.assert_array_equal(s.groups_of(ids[200:]), groups[200:])
    assert s.group_stats()["ids"] == 5000 and s.group_stats()["entries"] == 5000
    # ... also where the occurrences disagree on grouped / ungrouped, and for new ids
    fresh = np.array([3, 4], dtype=np.int64)
    s.set_groups(np.array([3, 4, 3, 4, 3], dtype=np.int64), np.array([5, -1, -1, 6, 7], dtype=np.int64))
    np.testing.assert_array_equal(s.groups_of(fresh), [7, 6])
    assert s.group_stats()["ids"] == 5002 and s.group_stats()["entries"] == 5002
    # ungrouping: the entry stays, the id has no group; the side slot too
    gone = np.concatenate([ids[1000:1100], [I64.min] if I64.min not in ids[1000:1100] else []]).astype(np.int64)
    s.set_groups(gone, np.full(len(gone), -1, dtype=np.int64))
    st = s.group_stats()
    assert st["ids"] == 5002 - len(gone) and st["entries"] == 5002
    assert (s.groups_of(gone) == -1).all()
    s.set_groups(gone, np.full(len(gone), -1, dtype=np.int64))  # again: nothing to count
    assert s.group_stats()["ids"] == 5002 - len(gone)
    # re-grouping
    s.set_groups(gone[:50], np.arange(50, dtype=np.int64))
    s.set_groups(gone[-1:], np.array([11], dtype=np.int64))
    st = s.group_stats()
    assert st["ids"] == 5002 - len(gone) + 51 and st["entries"] == 5002
    np.testing.assert_array_equal(s.groups_of(gone[:50]), np.arange(50))
    assert s.groups_of([I64.min])[0] == 11
    # a refused batch changes nothing
    with pytest.raises(pa.PcvError):
        s.set_groups([1, 2], [5, -2])
    np.testing.assert_array_equal(s.groups_of([1, 2]), groups[np.isin(ids, [1, 2])][np.argsort(ids[np.isin(ids, [1, 2])])])
    # clear: as created, and usable
    s.clear_groups()
    assert s.group_stats() == {"ids": 0, "entries": 0, "slots": 0, "rehashes": 0, "last_set_ms": 0.0}
    assert (s.groups_of(ids[:100]) == -1).all() and s.groups_of([I64.min])[0] == -1
    s.set_groups(ids[:10], groups[:10])
    st = s.group_stats()
    assert (st["ids"], st["entries"], st["slots"], st["rehashes"]) == (10, 10, 1024, 0)
    np.testing.assert_array_equal(s.groups_of(ids[:12]), np.concatenate([groups[:10], [-1, -1]]))
    s.close()


# ---- 2. long probe chains and wrap-around ------------------------------------------------------------------------------------
def test_probe_chains_wrap_around(ctx, oracle):
    dim = 64
    s = pa.Searcher(ctx, dim, "cosine")
    s.set_groups([I64.max], [0])
    slots = s.group_stats()["slots"]
    assert slots == 1024
    mask = slots - 1
    rng = np.random.default_rng(2)
    cand = rng.integers(I64.min + 1, I64.max, size=200_000, dtype=np.int64)
    chain = np.unique(cand[id_hash(cand, mask) == mask - 3])[:48]
    assert len(chain) == 48  # 48 ids from slot mask - 3 on: the chain runs past the end of the table into slots 0 ..
    other = cand[:48]
    ids = np.concatenate([chain, other])
    assert len(np.unique(ids)) == 96
    groups = np.concatenate([np.arange(48) // 4, 100 + np.arange(48) // 4]).astype(np.int64)
    order = rng.permutation(96)
    s.set_groups(ids[order], groups[order])
    st = s.group_stats()
    assert (st["slots"], st["entries"], st["ids"], st["rehashes"]) == (1024, 97, 97, 0)
    np.testing.assert_array_equal(s.groups_of(ids), groups)
    absent = np.unique(cand[id_hash(cand, mask) == mask - 3])[48:60]  # the same chain, walked to its end
    assert len(absent) and (s.groups_of(absent) == -1).all()
    # rows carrying those ids collapse by them
    rows = rng.standard_normal((96, dim)).astype(np.float32)
    s.add_rows(1, rows, ids)
    s.finalize()
    queries = rng.standard_normal((4, dim)).astype(np.float32)
    ref = GroupedReference(oracle, queries, rows, ids, "cosine")
    table = dict(zip(ids.tolist(), groups.tolist()))
    got = s.search_grouped(None, 25, queries)
    for q in range(4):
        want = ref.walk(q, 25, default_pool(25), table)
        assert len(want[0]) == 24 and want[4] == 96 and want[3].sum() == 72  # 24 groups of 4 rows each, and no 25th
        check(got, want, q, 25)
    s.close()


# ---- 3. planted documents, both metrics, every screen form -------------------------------------------------------------------
N_DOCS = 40


def document_corpus(metric, seed=7, n=3000, dim=D):
    """40 documents of 2 .. 30 rows round a centre each (cosine about 0.96 to it), 200 rows without a group, the other rows in
    groups of three by id; one id with a group on two rows of document 0, one id without a group on two rows next to centre 1.
    -> rows, ids, {id: group}, centres, rows of each document and, behind them, the two rows next to centre 1"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((N_DOCS, dim)).astype(np.float32)
    sizes = rng.integers(2, 31, size=N_DOCS)
    sizes[0], sizes[1] = 30, 2
    parts, doc_of = [], []
    for d in range(N_DOCS):
        parts.append(centres[d] + 0.3 * rng.standard_normal((sizes[d], dim)).astype(np.float32))
        doc_of += [d] * int(sizes[d])
    twins = centres[1] + 0.3 * rng.standard_normal((2, dim)).astype(np.float32)  # two rows, one id, no group
    n_fill = n - len(doc_of) - 2
    rows = np.concatenate(parts + [twins, rng.standard_normal((n_fill, dim)).astype(np.float32)]).astype(np.float32)
    doc_of = np.array(doc_of + [-1] * (n - len(doc_of)))
    ids = (rng.permutation(n) * 5 + 100).astype(np.int64)
    n_doc = int(sizes.sum())
    ids[1] = ids[0]                    # two rows of document 0 share an id (and its group)
    ids[n_doc + 1] = ids[n_doc]        # the twins share an id that has no group
    perm = rng.permutation(n)
    rows, ids, doc_of = rows[perm], ids[perm], doc_of[perm]
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(n, 1))).astype(np.float32)
    table = {}
    twin_id = int(ids[np.nonzero(perm == n_doc)[0][0]])
    fill = np.nonzero(doc_of < 0)[0]
    for j, r in enumerate(fill[200:]):  # (the first 200 of the others stay without a group)
        if int(ids[r]) != twin_id:
            table[int(ids[r])] = 1000 + j // 3
    for r in np.nonzero(doc_of >= 0)[0]:
        table[int(ids[r])] = int(doc_of[r])
    assert twin_id not in table and (ids == twin_id).sum() == 2
    doc_rows = [np.nonzero(doc_of == d)[0] for d in range(N_DOCS)]
    doc_rows.append(np.nonzero(ids == twin_id)[0])  # (last: the twins)
    return np.ascontiguousarray(rows), ids, table, centres, doc_rows


def document_queries(metric, centres, seed=19):
    rng = np.random.default_rng(seed)
    queries = (centres + 0.1 * rng.standard_normal(centres.shape)).astype(np.float32)
    if metric == "dot":
        queries = (queries * rng.uniform(0.5, 1.5, size=(len(queries), 1))).astype(np.float32)
    return queries


def set_table(s, table):
    s.set_groups(np.fromiter(table.keys(), dtype=np.int64), np.fromiter(table.values(), dtype=np.int64))


@pytest.fixture(scope="module")
def documents(oracle):
    out = {}
    for metric in ("cosine", "dot"):
        rows, ids, table, centres, doc_rows = document_corpus(metric)
        queries = document_queries(metric, centres)
        ref = GroupedReference(oracle, queries, rows, ids, metric)
        # what the cases rely on: query d meets the whole of document d before any other row — the cluster radius against the
        # gap to the next document — so its first hit stands for the document
        # (query 1 meets the two rows without a group there too, among the two of its document)
        for d in range(N_DOCS):
            L, _sc = ref.ranked(d)
            near = set(doc_rows[d].tolist()) | (set(doc_rows[N_DOCS].tolist()) if d == 1 else set())
            assert set(L[: len(near)].tolist()) == near, (metric, d)
            w = ref.walk(d, 10, default_pool(10), table)
            at = w[2].tolist().index(d)
            assert at <= (2 if d == 1 else 0) and w[3][at] == len(doc_rows[d]) - 1 and len(w[0]) == 10 and not w[5]
        out[metric] = (rows, ids, table, queries, ref)
    return out


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("form", list(FORMS))
def test_planted_documents(ctx, documents, form, metric):
    rows, ids, table, queries, ref = documents[metric]
    s = build_three_segments(ctx, metric, rows, ids, FORMS[form])
    set_table(s, table)
    assert s.group_stats()["ids"] == len(table)
    for B in (1, N_DOCS):
        for k in (1, 10, 128):
            got = s.search_grouped(None, k, queries[:B])
            for q in range(B):
                check(got, ref.walk(q, k, default_pool(k), table), q, k)
            if k == 10:
                scores_match_plain_search(s, got, queries[:B])
    # the two rows of document 0 with one id count as any two of its rows; the twins next to centre 1 are both kept
    w = ref.walk(1, 10, 128, table)
    twin = [i for i in w[0].tolist() if (ids == i).sum() == 2]
    assert len(twin) == 2 and twin[0] == twin[1] and (w[2][[w[0].tolist().index(twin[0])]] == -1).all()
    # a source filter: only the rows of source 2
    allowed = np.arange(2000, rows.shape[0])
    got = s.search_grouped([2], 10, queries[:8], pool=200)
    for q in range(8):
        check(got, ref.walk(q, 10, 200, table, allowed), q, 10)
    empty = s.search_grouped([], 10, queries[:3])  # an empty filter matches nothing
    assert (empty[3] == 0).all() and (empty[0] == -1).all() and (empty[5] == 0).all() and not empty[6].any()
    s.close()


# ---- 4. padded width and a list shorter than a pass --------------------------------------------------------------------------
def test_padded_width_and_short_list(ctx, oracle):
    n, dim = 77, 100  # the shape of the golden fixture
    rng = np.random.default_rng(4)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    ids = (rng.permutation(n) + 500).astype(np.int64)
    queries = rng.standard_normal((3, dim)).astype(np.float32)
    table = {int(i): int(i) % 8 for i in ids}  # eight groups: fewer than the ten asked for
    s = pa.Searcher(ctx, dim, "cosine")
    s.add_rows(1, rows, ids)
    s.finalize()
    set_table(s, table)
    ref = GroupedReference(oracle, queries, rows, ids, "cosine")
    got = s.search_grouped(None, 10, queries)
    for q in range(3):
        want = ref.walk(q, 10, 128, table)
        assert len(want[0]) == 8 and want[4] == 77 and not want[5] and want[3].sum() == 69
        check(got, want, q, 10)
    assert (got[5] == 77).all() and not got[6].any()
    scores_match_plain_search(s, got, queries)
    got = s.search_grouped(None, 8, queries, pool=77)  # the pool ends where the list ends: nothing more
    for q in range(3):
        check(got, ref.walk(q, 8, 77, table), q, 8)
    got = s.search_grouped(None, 10, queries, pool=76)  # ... and one before
    for q in range(3):
        want = ref.walk(q, 10, 76, table)
        assert want[5] and want[4] == 76
        check(got, want, q, 10)
    s.close()


# ---- 5. passes and the pool limit --------------------------------------------------------------------------------------------
def test_passes_and_pool_limit(ctx, oracle):
    n, big = 3000, 300
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    queries = rng.standard_normal((6, D)).astype(np.float32)
    u = queries[0] / np.linalg.norm(queries[0])
    for q in range(1, 6):  # the other queries point away from query 0: its document is at the end of their lists
        queries[q] -= (queries[q] @ u + 0.3 * np.linalg.norm(queries[q])) * u
    noise = rng.standard_normal((big, D))
    noise -= np.outer(noise @ u, u)
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    at = rng.choice(n, size=big, replace=False)
    rows[at] = (np.linalg.norm(queries[0]) * (u + 0.1 * noise)).astype(np.float32)  # cosine 0.995 with query 0
    ids = (rng.permutation(n) * 3 + 7).astype(np.int64)
    table = {int(i): 42 for i in ids[at]}  # one document of 300 rows; every other row is a group of its own
    s = pa.Searcher(ctx, D, "cosine")
    s.add_rows(1, rows[:1700], ids[:1700])
    s.add_rows(2, rows[1700:], ids[1700:])
    s.finalize()
    set_table(s, table)
    ref = GroupedReference(oracle, queries, rows, ids, "cosine", depth=1000)
    L0, _sc = ref.ranked(0)
    assert set(L0[:big].tolist()) == set(at.tolist())  # query 0's first 300 list entries are the planted document
    for q in range(1, 6):
        assert not np.isin(ref.ranked(q)[0][:5], at).any()  # the others finish with their first five rows
    narrow = s.search_grouped(None, 5, queries, pool=128)
    for q in range(6):
        check(narrow, ref.walk(q, 5, 128, table), q, 5)
    assert narrow[3][0] == 1 and narrow[4][0, 0] == 127 and narrow[5][0] == 128 and narrow[6][0] and narrow[2][0, 0] == 42
    assert (narrow[5][1:] == 5).all() and not narrow[6][1:].any()
    wide = s.search_grouped(None, 5, queries, pool=512)
    for q in range(6):
        check(wide, ref.walk(q, 5, 512, table), q, 5)
    assert wide[3][0] == 5 and wide[4][0, 0] == big - 1 and wide[5][0] == big + 4 and not wide[6][0]  # rows of three passes counted
    odd = s.search_grouped(None, 5, queries, pool=300)  # pool mod 128 != 0: the third pass lists 44 hits
    for q in range(6):
        check(odd, ref.walk(q, 5, 300, table), q, 5)
    assert odd[3][0] == 1 and odd[4][0, 0] == 299 and odd[5][0] == 300 and odd[6][0]
    odd = s.search_grouped(None, 5, queries, pool=301)
    check(odd, ref.walk(0, 5, 301, table), 0, 5)
    assert odd[3][0] == 2 and odd[5][0] == 301 and odd[6][0]
    scores_match_plain_search(s, wide, queries)
    # the finished queries are left alone by the passes query 0 goes on to: as in a call without it
    rest = s.search_grouped(None, 5, queries[1:], pool=512)
    for a, b in zip(wide, rest):
        np.testing.assert_array_equal(bits(a[1:]) if a.dtype == np.float32 else a[1:], bits(b) if b.dtype == np.float32 else b)
    s.close()


# ---- 6. more queries than one pass takes -------------------------------------------------------------------------------------
def test_more_queries_than_one_pass(ctx, oracle):
    n, nq, k = 1000, 300, 10
    rng = np.random.default_rng(6)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = np.arange(n, dtype=np.int64) + 10
    queries = rng.standard_normal((nq, D)).astype(np.float32)
    table = {int(i): int(i) // 8 for i in ids[: n - 100]}  # groups of eight; the last hundred rows have none
    s = pa.Searcher(ctx, D, "cosine")
    s.add_rows(1, rows, ids)
    s.finalize()
    set_table(s, table)
    got = s.search_grouped(None, k, queries)
    assert got[0].shape == (nq, k) and (got[3] == k).all()
    assert got[4].sum() > 0  # (rows did collapse)
    for q in range(nq):
        one = s.search_grouped(None, k, queries[q : q + 1])
        for a, b in zip(got, one):
            np.testing.assert_array_equal(bits(a[q : q + 1]) if a.dtype == np.float32 else a[q : q + 1], bits(b) if b.dtype == np.float32 else b)
    ref = GroupedReference(oracle, queries[::37], rows, ids, "cosine", depth=200)
    for j, q in enumerate(range(0, nq, 37)):
        w = ref.walk(j, k, 128, table)
        np.testing.assert_array_equal(got[0][q], w[0])
        np.testing.assert_array_equal(bits(got[1][q]), bits(w[1]))
        np.testing.assert_array_equal(got[4][q], w[3])
        assert got[5][q] == w[4]
    s.close()


# ---- 7. ties -----------------------------------------------------------------------------------------------------------------
def test_ties_go_by_position(ctx, oracle):
    rng = np.random.default_rng(8)
    n = 400
    rows = rng.standard_normal((n, D)).astype(np.float32)
    query = rng.standard_normal((1, D)).astype(np.float32)
    same = (query[0] + 0.2 * rng.standard_normal(D)).astype(np.float32)
    pair = (query[0] + 0.4 * rng.standard_normal(D)).astype(np.float32)
    four, two = [310, 20, 170, 90], [250, 60]
    rows[four] = same  # four bit-identical rows in four groups
    rows[two] = pair   # two bit-identical rows in one group
    ids = (rng.permutation(n) + 1).astype(np.int64)
    table = {int(ids[r]): 10 + j for j, r in enumerate(four)}
    table.update({int(ids[r]): 99 for r in two})
    s = pa.Searcher(ctx, D, "cosine")
    s.add_rows(1, rows[:200], ids[:200])
    s.add_rows(1, rows[200:], ids[200:])
    s.finalize()
    set_table(s, table)
    ref = GroupedReference(oracle, query, rows, ids, "cosine")
    want = ref.walk(0, 6, 128, table)
    # the order is by position; inside the group the lower position stands for it and the other is collapsed into it
    assert want[0][:5].tolist() == [int(ids[r]) for r in sorted(four)] + [int(ids[min(two)])]
    assert want[2][:5].tolist() == [table[int(ids[r])] for r in sorted(four)] + [99] and want[3][:5].tolist() == [0, 0, 0, 0, 1]
    assert len(set(bits(want[1][:4]).tolist())) == 1
    got = s.search_grouped(None, 6, query)
    check(got, want, 0, 6)
    got = s.search_grouped(None, 5, query)  # the walk ends with the group's first row: its twin is not examined
    check(got, ref.walk(0, 5, 128, table), 0, 5)
    assert got[4][0, 4] == 0 and got[5][0] == 5
    s.close()


# ---- 8. hidden, removed and updated items, a view, search by example ---------------------------------------------------------
def test_changes_views_and_like(ctx, oracle, documents):
    metric = "cosine"
    rows, ids, table, queries, _ref = documents[metric]
    queries = queries[:8]
    n = rows.shape[0]
    K, POOL = 10, 256
    s = build_three_segments(ctx, metric, rows, ids, ("auto", "auto", "auto", 0))
    set_table(s, table)

    def same_as_fresh(cur_rows, cur_ids, groups, allowed=None, searcher=None):
        ref = GroupedReference(oracle, queries, cur_rows, cur_ids, metric, depth=700)
        got = (searcher or s).search_grouped(None, K, queries, pool=POOL)
        for q in range(len(queries)):
            check(got, ref.walk(q, K, POOL, groups, allowed), q, K)
        return got

    base = same_as_fresh(rows, ids, table)
    first = [q for q in range(8) if q != 1]  # (query 1 may meet the two rows without a group before its document)
    assert (base[2][first, 0] == first).all() and (base[4][first, 0] >= 1).all()  # query d: document d first
    # a hidden best member: the next member stands for its group, and counts one row fewer
    hit = [q for q in (0, 2, 3) if (ids == base[0][q, 0]).sum() == 1]
    best = base[0][hit, 0].copy()
    assert len(best) >= 2
    s.hide_items(best)
    got = same_as_fresh(rows, ids, table, allowed=np.nonzero(~np.isin(ids, best))[0])
    assert not np.isin(got[0], best).any()
    for q in hit:
        assert got[2][q, 0] == base[2][q, 0] and got[4][q, 0] == base[4][q, 0] - 1 and got[0][q, 0] != base[0][q, 0]
    s.unhide_items(best)
    again = same_as_fresh(rows, ids, table)
    np.testing.assert_array_equal(again[0], base[0])
    # an updated member moves: its group does not
    moved = [int(np.nonzero(ids == base[0][q, 0])[0][0]) for q in (4, 5)]
    new_rows = rows.copy()
    new_rows[moved] = rows[moved][::-1]  # the best rows of documents 4 and 5 swap places
    s.update_items(ids[moved], new_rows[moved])
    got = same_as_fresh(new_rows, ids, table)
    # (query 4 now meets the id of document 5 first, which kept its group)
    assert got[0][4, 0] == base[0][5, 0] and got[2][4, 0] == 5 and got[0][5, 0] == base[0][4, 0] and got[2][5, 0] == 4
    # a view over half of the ids reads the parent's groups
    half = ids[::2]
    in_view = np.nonzero(np.isin(ids, half))[0]
    v = s.view(half)
    same_as_fresh(new_rows, ids, table, allowed=in_view, searcher=v)
    np.testing.assert_array_equal(v.groups_of(ids[:50]), s.groups_of(ids[:50]))
    assert v.group_stats() == s.group_stats()
    for change in (lambda: v.set_groups([1], [2]), lambda: v.clear_groups()):
        with pytest.raises(pa.PcvError) as err:
            change()
        assert "the searcher is a view (read-only)" in str(err.value)
    # ... at call time: a set_groups on the parent between two searches of the view
    merged = dict(table)
    for i in ids[np.isin(ids, [i for i, g in table.items() if g in (0, 1)])]:
        merged[int(i)] = 0  # documents 0 and 1 become one
    set_table(s, {i: g for i, g in merged.items() if table[i] != g})
    got = same_as_fresh(new_rows, ids, merged, allowed=in_view, searcher=v)
    assert 0 in got[2][1, :3] and 1 not in got[2][1]
    v.close()
    # search by example: the item itself first, then the groups round it
    item = int(base[0][2, 0])
    row_of = int(np.nonzero(ids == item)[0][0])
    items = s.search_grouped_like_item(None, K, item, pool=POOL)
    ref1 = GroupedReference(oracle, new_rows[row_of : row_of + 1], new_rows, ids, metric, depth=700)
    w = ref1.walk(0, K, POOL, merged)
    assert items[0][0].id == item and [it.id for it, _g, _c in items] == [int(x) for x in w[0]] and len(items) == K
    np.testing.assert_array_equal(bits([it.score for it, _g, _c in items]), bits(w[1]))
    assert [g for _it, g, _c in items] == w[2].tolist() and [c for _it, _g, c in items] == w[3].tolist()
    with pytest.raises(KeyError):
        s.search_grouped_like_item(None, K, -12345)
    # removed items: the groups follow the ids through the compaction, and an id that comes back has its group again
    gone = ids[np.r_[5:40, 1990:2020, n - 7 : n]]
    gone = gone[[(ids == g).sum() == 1 for g in gone]]
    s.remove_items(gone)
    stay = ~np.isin(ids, gone)
    same_as_fresh(new_rows[stay], ids[stay], merged)
    np.testing.assert_array_equal(s.groups_of(gone), [merged.get(int(i), -1) for i in gone])
    s.add_rows(2, new_rows[~stay], ids[~stay])
    s.finalize()
    back = np.concatenate([np.nonzero(stay)[0], np.nonzero(~stay)[0]])
    same_as_fresh(new_rows[back], ids[back], merged)
    s.close()


# ---- 9. an empty table -------------------------------------------------------------------------------------------------------
def test_empty_table_is_the_plain_search(ctx):
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((700, D)).astype(np.float32)
    queries = rng.standard_normal((5, D)).astype(np.float32)
    s = pa.Searcher(ctx, D, "dot")
    s.add_rows(1, rows, np.arange(700) * 2)
    s.finalize()

    def plain_equal():
        for k in (1, 10, 128):
            ids, scores, groups, counts, collapsed, examined, more = s.search_grouped(None, k, queries)
            p_ids, p_scores, p_counts = s.search_vectors(None, k, queries)
            np.testing.assert_array_equal(ids, p_ids)
            np.testing.assert_array_equal(bits(scores), bits(p_scores))
            np.testing.assert_array_equal(counts, p_counts)
            assert (groups == -1).all() and (collapsed == 0).all() and (examined == k).all() and not more.any()

    plain_equal()                       # never set
    s.set_groups([1, 3, 5], [0, 0, 0])  # ids no row carries
    plain_equal()
    s.set_groups(np.arange(700) * 2, np.full(700, -1))  # entries without a group
    plain_equal()
    s.clear_groups()
    plain_equal()
    s.close()


# ---- 10. the refusals --------------------------------------------------------------------------------------------------------
def test_unfinalized_searcher_gives_the_error_of_search(ctx):
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((40, 32)).astype(np.float32)
    s = pa.Searcher(ctx, 32, "cosine")
    s.add_rows(1, rows, np.arange(40))
    s.set_groups(np.arange(40), np.arange(40) // 4)  # (the table does not wait for finalize)
    with pytest.raises(pa.PcvError) as plain:
        s.search_vectors(None, 5, rows[:1])
    with pytest.raises(pa.PcvError) as grouped:
        s.search_grouped(None, 5, rows[:1])
    assert grouped.value.status == plain.value.status
    tail = "rows were added or cleared without pcv_searcher_finalize"
    assert str(plain.value).endswith(tail) and str(grouped.value).endswith("search_grouped: " + tail)
    s.finalize()
    ids, _scores, groups, counts, collapsed, examined, more = s.search_grouped(None, 5, rows[:1])
    assert counts[0] == 5 and ids[0, 0] == 0 and groups[0, 0] == 0 and not more[0] and examined[0] >= 5
    assert examined[0] == 5 + collapsed[0].sum()
    s.close()


# ---- 11. the C++ mirror ------------------------------------------------------------------------------------------------------
def test_cpp_mirror_grouped_program():
    src = os.path.join(ROOT, "tests", "cpp", "grouped_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "grouped_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "grouped_mirror_test: ok" in r.stdout
