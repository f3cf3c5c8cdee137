"""GPU: search by example (pcv_searcher_like_queries / _search_like).  The vectors are compared with the stored rows (bit for bit
for one example, against an f64 sum with the bound of n sequential f32 fused multiply-adds for weighted groups), the searches with
pcv_searcher_search of those vectors (bit for bit: ids, scores, counts) and with the oracle over the rows that remain."""
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from perceive_amd.sharded import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

METRIC = {"cosine": 0, "dot": 1}
PCV_ERR_INVALID = 1
D = 384
SYN0 = 500000  # first implicit id of the synthetic source
UNKNOWN = (-5, 7, 10**12)  # ids no row carries


@pytest.fixture(scope="module")
def g1000(golden_dir):
    return np.load(os.path.join(golden_dir, "scan_n1000_d384.npz"))


def golden_parts(g1000):
    """two sources with permuted explicit ids; id A is carried by a row of each source, id B by two rows of source 1"""
    corpus = g1000["corpus"]
    ids = (np.random.default_rng(7).permutation(1000) * 3 + 100011).astype(np.int64)
    ids[600] = ids[5]
    ids[20] = ids[10]
    return [(1, corpus[:600], ids[:600].copy()), (2, corpus[600:], ids[600:].copy())], ids


def build(ctx, metric, parts, screen="auto", synthetic=300):
    s = pa.Searcher(ctx, D, metric)
    s.set_screening_copy(screen)
    for src, rows, ids in parts:
        s.add_rows(src, rows, ids)
    if synthetic:
        s.add_synthetic(3, synthetic, 9, first_row=SYN0)  # implicit ids SYN0 + row
    s.finalize()
    return s


def table(s):
    """every stored row and its id, by global position (what pcv_searcher_get_rows returns)"""
    return s.get_rows(np.arange(s.num_rows))


def source_of(s):
    """source id of every global position"""
    return np.concatenate([np.full(s.source_num_rows(x), x, dtype=np.int64) for x in s.source_ids])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(bits(a[1]), bits(b[1]))
    np.testing.assert_array_equal(a[2], b[2])


def drop_own(res, groups, k):
    """(ids, scores, counts) of a longer search with each query's own example ids dropped and the rest cut to k"""
    ids, scores, counts = res
    B = ids.shape[0]
    oi = np.full((B, k), -1, dtype=np.int64)
    os_ = np.full((B, k), np.nan, dtype=np.float32)
    oc = np.zeros(B, dtype=np.int32)
    for q in range(B):
        own = set(int(x) for x in groups[q])
        keep = [j for j in range(int(counts[q])) if int(ids[q, j]) not in own][:k]
        oi[q, : len(keep)] = ids[q, keep]
        os_[q, : len(keep)] = scores[q, keep]
        oc[q] = len(keep)
    return oi, os_, oc


def reference(rows, ids, groups, weights):
    """the defined sum in f64: examples in the order given, an example's rows in ascending position; and sum |w x| per component"""
    B = len(groups)
    ref = np.zeros((B, D))
    mag = np.zeros((B, D))
    members = np.zeros(B, dtype=np.int64)
    found = []
    for q, g in enumerate(groups):
        for i, e in enumerate(g):
            at = np.flatnonzero(ids == e)
            found.append(at.size > 0)
            w = float(np.float32(1.0 if weights is None else weights[q][i]))
            for r in at:
                ref[q] += w * rows[r].astype(np.float64)
                mag[q] += np.abs(w * rows[r].astype(np.float64))
            members[q] += at.size
    return ref, mag, members, np.array(found, dtype=bool)


def single_ids(ids, n, seed):
    """n distinct ids each carried by exactly one row"""
    u, c = np.unique(ids, return_counts=True)
    return np.random.default_rng(seed).choice(u[c == 1], n, replace=False)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_single_example_is_the_stored_row(ctx, g1000, metric):
    parts, _ = golden_parts(g1000)
    s = build(ctx, metric, parts)
    rows, ids = table(s)
    pick = np.concatenate([single_ids(ids[:1000], 60, 1), [SYN0, SYN0 + 299, SYN0 + 31, SYN0 + 32]])
    groups = [[int(x)] for x in pick]
    d_out = ctx.alloc(len(groups) * D * 4)
    vec, found, members = s.like_queries(groups, d_out=d_out)
    dev = ctx.to_host(d_out, len(groups) * D * 4).view(np.float32).reshape(len(groups), D)
    want = np.stack([rows[np.flatnonzero(ids == x)[0]] for x in pick])
    np.testing.assert_array_equal(bits(vec), bits(want))
    np.testing.assert_array_equal(bits(dev), bits(want))
    assert found.all() and (members == 1).all()
    again, _, _ = s.like_queries(groups, weights=[[1.0]] * len(groups))
    np.testing.assert_array_equal(bits(again), bits(vec))
    ctx.free(d_out)
    s.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
def weighted_groups(ids, hidden_id, seed):
    rng = np.random.default_rng(seed)
    multi = [int(ids[5]), int(ids[10])]  # carried by two rows each
    groups, weights = [], []
    for n in (2, 3, 17, 64, 150, 300):
        g = [int(x) for x in rng.choice(ids, n - 1)] + [multi[n % 2]]
        if n > 2:
            g[n // 2] = g[0]  # an id listed twice
        if n >= 17:
            g[3] = UNKNOWN[n % 3]
            g[4] = hidden_id
            g[5] = SYN0 + n
        w = rng.choice(np.array([1, -1, 0.25], dtype=np.float32), n) if n % 2 else rng.standard_normal(n).astype(np.float32)
        groups.append(g)
        weights.append(w)
    return groups, weights


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_weighted_groups(ctx, g1000, metric):
    parts, _ = golden_parts(g1000)
    s = build(ctx, metric, parts)
    rows, ids = table(s)
    hidden_id = int(single_ids(ids[:1000], 1, 2)[0])
    assert s.hide_items([hidden_id]) == 1
    groups, weights = weighted_groups(ids, hidden_id, 3)
    vec, found, members = s.like_queries(groups, weights)
    ref, mag, ref_members, ref_found = reference(rows, ids, groups, weights)
    np.testing.assert_array_equal(members, ref_members)
    np.testing.assert_array_equal(found, ref_found)
    assert not found.all() and members[0] >= 3 and members[1] >= 4  # unknown ids; an id with two rows
    for q in range(len(groups)):
        bound = (members[q] + 1) * 2.0 ** -24 * mag[q]  # n sequential f32 fused multiply-adds
        err = np.abs(vec[q].astype(np.float64) - ref[q])
        print(f"group of {len(groups[q])}: max err {err.max():.3e}, bound there {bound[err.argmax()]:.3e}")
        assert (err <= bound).all()
    again, found2, members2 = s.like_queries(groups, weights)
    np.testing.assert_array_equal(bits(again), bits(vec))
    np.testing.assert_array_equal(found2, found)
    np.testing.assert_array_equal(members2, members)
    s.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
def search_groups(ids, B, seed):
    """B groups: single examples, and every fourth a small weighted group with an id two rows carry"""
    rng = np.random.default_rng(seed)
    groups, weights = [], []
    for q in range(B):
        if q % 4 == 3:
            g = [int(x) for x in rng.choice(ids, 3)] + [int(ids[5 if q % 8 == 3 else 10])]
            w = [1.0, 0.5, -0.25, 1.0]
        else:
            g, w = [int(rng.choice(ids))], [1.0]
        groups.append(g)
        weights.append(np.array(w, dtype=np.float32))
    return groups, weights


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("screen", ["int8", "bf16", "off"])
def test_search_equals_search_of_the_vector(ctx, oracle, g1000, screen, metric):
    parts, _ = golden_parts(g1000)
    s = build(ctx, metric, parts, screen=screen)
    rows, ids = table(s)
    src = source_of(s)
    for B in (1, 4, 64, 256):
        groups, weights = search_groups(ids, B, 10 + B)
        v, found, members = s.like_queries(groups, weights)
        assert found.all()
        m_max = int(members.max())
        for k in (10, 129, 1000):
            for sources in (None, [1, 3]):
                got = s.search_like(sources, k, groups, weights, exclude_examples=False)
                assert_same(got[:3], s.search_vectors(sources, k, v))
                assert got[3].all()
                got = s.search_like(sources, k, groups, weights, exclude_examples=True)
                assert_same(got[:3], drop_own(s.search_vectors(sources, k + m_max, v), groups, k))
                # the oracle over the selected rows minus the query's member rows
                sel = np.ones(ids.size, dtype=bool) if sources is None else np.isin(src, sources)
                for q in range(B):
                    keep = sel & ~np.isin(ids, groups[q])
                    opos, _, ocnt = oracle.topk(v[q:q + 1], rows[keep], k, METRIC[metric])
                    kid = ids[keep]
                    np.testing.assert_array_equal(got[0][q], np.where(opos[0] >= 0, kid[np.maximum(opos[0], 0)], -1))
                    assert got[2][q] == ocnt[0]  # (below k only when fewer searchable rows remain: the oracle counts them)
    s.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_reference_case(ctx, g1000):
    parts, _ = golden_parts(g1000)
    s = build(ctx, "dot", parts)
    rows, ids = table(s)
    for item in [int(x) for x in single_ids(ids[:1000], 5, 4)] + [SYN0 + 7]:
        row = rows[np.flatnonzero(ids == item)[0]]
        hits = s.search_like_item(None, 20, item)
        assert len(hits) == 20 and hits[0].id == item
        dist = max(0.0, 1.0 - float((row.astype(np.float64) ** 2).sum()) / D)  # search.rs:269-278
        assert abs(hits[0].score - dist) <= 2.0 ** -23 * max(dist, 2.0 ** -126)
        assert hits == s.search_vector(None, 20, row)
        assert [h.id for h in s.search_like_item(None, 19, item, exclude=True)] == [h.id for h in hits[1:]]
    with pytest.raises(KeyError, match="Item not found"):
        s.search_like_item(None, 20, UNKNOWN[0])
    s.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_not_found_and_empty(ctx, g1000, metric):
    parts, _ = golden_parts(g1000)
    s = build(ctx, metric, parts)
    _, ids = table(s)
    a, b = (int(x) for x in single_ids(ids[:1000], 2, 5))
    groups = [[a], [UNKNOWN[0], UNKNOWN[1]], [], [b, UNKNOWN[2]]]
    for exclude in (False, True):
        got = s.search_like(None, 10, groups, exclude_examples=exclude)
        alone = s.search_like(None, 10, [[a], [b]], exclude_examples=exclude)
        for q in (1, 2):
            assert got[2][q] == 0 and (got[0][q] == -1).all() and np.isnan(got[1][q]).all()
        assert_same([x[[0, 3]] for x in got[:3]], alone[:3])
        assert got[3].tolist() == [True, False, False, True, False]
    vec, found, members = s.like_queries(groups)
    assert members.tolist() == [1, 0, 0, 1] and not vec[1].any() and not vec[2].any()
    assert (bits(vec[1:3]) == 0).all()
    # nothing to do
    vec, found, members = s.like_queries([])
    assert vec.shape == (0, D) and found.size == 0 and members.size == 0
    got = s.search_like(None, 10, [])
    assert got[0].shape == (0, 10) and got[2].size == 0
    got = s.search_like(None, 10, [[UNKNOWN[0]], []])  # no query has a member
    assert (got[2] == 0).all() and (got[0] == -1).all() and np.isnan(got[1]).all()
    s.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_views_look_examples_up_in_the_parent(ctx, g1000, metric):
    parts, _ = golden_parts(g1000)
    s = build(ctx, metric, parts)
    rows, ids = table(s)
    src = source_of(s)
    rng = np.random.default_rng(6)
    allow = rng.choice(np.unique(ids), 400, replace=False)
    inside = [int(x) for x in allow[:6]]
    outside = [int(x) for x in np.setdiff1d(ids, allow)[:6]]
    groups = [[x] for x in inside + outside] + [[inside[0], outside[0], int(ids[5])], [outside[1], outside[2]]]
    weights = [np.ones(len(g), dtype=np.float32) for g in groups]
    weights[-2] = np.array([1.0, -0.5, 0.25], dtype=np.float32)
    v = s.view(allow)
    # a searcher built fresh from the allowed rows, in the parent's source and row order
    keep = np.isin(ids, allow)
    f = build(ctx, metric, [(int(x), rows[keep & (src == x)], ids[keep & (src == x)]) for x in s.source_ids if (keep & (src == x)).any()],
              synthetic=0)
    vec, found, members = s.like_queries(groups, weights)
    vvec, vfound, vmembers = v.like_queries(groups, weights)
    np.testing.assert_array_equal(bits(vvec), bits(vec))
    assert vfound.all() and (vmembers == members).all()
    m_max = int(members.max())
    for sources in (None, [2, 3]):
        for k in (10, 150):
            got = v.search_like(sources, k, groups, weights, exclude_examples=True)
            assert_same(got[:3], drop_own(f.search_vectors(sources, k + m_max, vec), groups, k))
            got = v.search_like(sources, k, groups, weights, exclude_examples=False)
            assert_same(got[:3], f.search_vectors(sources, k, vec))
            assert np.isin(got[0][got[0] >= 0], allow).all()
    hits = v.search_like_item(None, 5, outside[3])
    assert len(hits) == 5 and all(h.id in set(allow.tolist()) for h in hits)
    v.close()
    f.close()
    s.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_follows_changes_and_is_read_only(ctx, g1000):
    parts, _ = golden_parts(g1000)
    s = build(ctx, "cosine", parts)
    rows, ids = table(s)
    a, b, c = (int(x) for x in single_ids(ids[:1000], 3, 8))
    probe = g1000["queries"][:8]
    before = s.search_vectors(None, 10, probe)
    first = s.search_like(None, 10, [[a], [b], [c]])
    # update: the vector is the new row
    new = np.random.default_rng(9).standard_normal((1, D)).astype(np.float32)
    s.update_items([a], new)
    vec, found, _ = s.like_queries([[a]])
    np.testing.assert_array_equal(bits(vec), bits(new))
    s.update_items([a], rows[ids == a])
    # hide: the vector is unchanged, and the item is in no result even without exclusion
    s.hide_items([b])
    vec, found, members = s.like_queries([[b]])
    np.testing.assert_array_equal(bits(vec[0]), bits(rows[ids == b][0]))
    assert found[0] and members[0] == 1
    got = s.search_like(None, 10, [[b]], exclude_examples=False)
    assert b not in got[0] and got[2][0] == 10
    assert_same(got[:3], s.search_vectors(None, 10, vec))
    s.unhide_items([b])
    assert_same(s.search_like(None, 10, [[a], [b], [c]])[:3], first[:3])
    assert_same(s.search_vectors(None, 10, probe), before)  # the calls so far changed nothing
    # remove: the example is gone
    assert s.remove_items([c]) == 1
    vec, found, members = s.like_queries([[c], [a]])
    assert found.tolist() == [False, True] and members.tolist() == [0, 1] and not vec[0].any()
    got = s.search_like(None, 10, [[c]])
    assert got[2][0] == 0 and not got[3][0]
    s.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_state(ctx, g1000):
    parts, ids = golden_parts(g1000)
    s = build(ctx, "cosine", parts)
    g = [[int(ids[0])]]
    s.add_rows(1, g1000["corpus"][100:104], np.arange(4, dtype=np.int64))
    for call in (lambda: s.like_queries(g), lambda: s.search_like(None, 10, g)):
        with pytest.raises(pa.PcvError) as e:
            call()
        assert e.value.status == PCV_ERR_INVALID and "pending rows" in str(e.value)
    s.finalize()
    d_out = ctx.alloc((4 * 10 + 1) * HIT_DTYPE.itemsize)
    s.search_device_begin(None, 10, g1000["queries"][:4], d_out)
    for call in (lambda: s.like_queries(g), lambda: s.search_like(None, 10, g)):
        with pytest.raises(pa.PcvError) as e:
            call()
        assert e.value.status == PCV_ERR_INVALID and "queued pass" in str(e.value)
    s.search_device_end()
    assert s.search_like(None, 10, g, exclude_examples=False)[0][0, 0] == ids[0]
    ctx.free(d_out)
    s.close()


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_size(ctx):
    n_seg, seg = 4, 500_000  # 2M x 384 in four implicit-id segments of two sources, AUTO copies
    s = pa.Searcher(ctx, D, "cosine")
    for i in range(n_seg):
        s.add_synthetic(1 + i // 2, seg, 77, first_row=i * seg)
    s.finalize()
    assert s.num_rows == n_seg * seg and s.num_segments == n_seg
    pick = np.random.default_rng(10).choice(n_seg * seg, 64, replace=False).astype(np.int64)
    groups = [[int(x)] for x in pick]
    v, found, members = s.like_queries(groups)
    assert found.all() and (members == 1).all()
    rows, rid = s.get_rows(pick)  # implicit ids: position == id here
    np.testing.assert_array_equal(rid, pick)
    np.testing.assert_array_equal(bits(v), bits(rows))
    full = s.search_vectors(None, 11, v)
    np.testing.assert_array_equal(full[0][:, 0], pick)  # the example itself is rank 0 of the unfiltered list
    got = s.search_like(None, 10, groups, exclude_examples=True)
    assert_same(got[:3], drop_own(full, groups, 10))
    assert (got[2] == 10).all() and s.last_stats()["rows_scanned"] >= n_seg * seg
    s.close()


def test_cpp_mirror_like_program():
    src = os.path.join(ROOT, "tests", "cpp", "like_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "like_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "like_mirror_test: ok" in r.stdout
