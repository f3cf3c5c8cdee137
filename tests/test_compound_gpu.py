"""GPU: compound queries (pcv_searcher_search_compound / _search_compound_like), through the C ABI.  The reference of every check is
tests/compound_ref.py: oracle.topk over all rows gives every vector's ranked list and every row's canonical score, the walk in steps
of 128, the union without repeats, the strict certificate and the end of a list are Python written from the definition, and a brute
force over all rows stands beside them.  Ids, counts, examined and exact are compared for equality, combined scores and penalties by
their 64 bits, part scores by their 32 bits against the model and against search_vectors of the same vector at that row."""
import os
import subprocess

import numpy as np
import pytest

import compound_ref as cr
import perceive_amd as pa
from compound_ref import ALL, ANY, CASES, COMPOUNDS, COMPOUNDS_W8, LAMBDAS, bits32, bits64, check
from test_distinct_gpu import FORMS, SPLIT, build_three_segments, planted_corpus, planted_queries
from test_view_gpu import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384
MODES = {ALL: "all", ANY: "any"}


@pytest.fixture(scope="module")
def corpus(oracle):
    """per metric: the bridged corpus, the 24 vectors, the bridge ids, the model (lists computed once) and the walks it has made"""
    out = {}
    for metric in ("cosine", "dot"):
        rows, ids, anchors, bridge_ids = cr.bridged_corpus(planted_corpus, metric)
        vectors = cr.compound_vectors(planted_queries, metric, anchors)
        out[metric] = (rows, ids, vectors, bridge_ids, cr.CompoundReference(oracle, vectors, rows, ids, metric), {})
    return out


def compound(s, vectors, compounds, k, mode, lam, pool, sources=None):
    wants = [vectors[list(w)] for w, _a in compounds]
    avoids = [vectors[list(a)] for _w, a in compounds]
    return s.search_compound(sources, k, wants, avoids if any(len(a) for _w, a in compounds) else None, MODES[mode], lam, pool)


def model_walk(ref, walks, c, mode, lam, k, pool, allowed=None, tag=None):
    lam = lam if c[1] else 0.0  # (without avoided vectors the weight changes nothing: one walk serves)
    key = (c, mode, lam, k, pool, tag)
    if key not in walks:
        walks[key] = ref.walk(c[0], c[1], mode, lam, k, pool, allowed)
    return walks[key]


def model_brute(ref, walks, c, mode, lam, k, allowed=None, tag=None):
    lam = lam if c[1] else 0.0
    key = (c, mode, lam, k, "brute", tag)
    if key not in walks:
        walks[key] = ref.brute(c[0], c[1], mode, lam, k, allowed)
    return walks[key]


def plain_scores(s, vectors, ids):
    """{item id: reported f32 score} per vector, from search_vectors over the whole corpus: what out_part_scores is held against"""
    n = ids.shape[0]
    p_ids, p_scores, p_counts = s.search_vectors(None, n, vectors)
    assert (p_counts == n).all()
    return [dict(zip(p_ids[v].tolist(), bits32(p_scores[v]).tolist())) for v in range(vectors.shape[0])]


def check_parts_against_plain(got, plain, c, i):
    ids, _m, parts, _p, counts, _e, _x = got
    for r in range(int(counts[i])):
        for j, v in enumerate(c[0]):
            assert int(bits32(parts[i, r, j : j + 1])[0]) == plain[v][int(ids[i, r])], (i, r, j)


def plan(form):
    """(mode, avoid_weight, k, pool) of test_parity: the whole cross on the int8 form; elsewhere every (k, pool) under both modes at
    one weight, and the other two weights at a short and a long walk"""
    if form == "mfma_int8":
        return [(mode, lam, k, pool) for mode in (ALL, ANY) for lam in LAMBDAS for k, pool in CASES]
    return ([(mode, 0.5, k, pool) for mode in (ALL, ANY) for k, pool in CASES] +
            [(mode, lam, k, pool) for mode in (ALL, ANY) for lam in (0.0, 4.0) for k, pool in ((10, 128), (128, 4096))])


# ---- 1. parity with the model, every form, both metrics ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("form", list(FORMS))
def test_parity(ctx, corpus, form, metric):
    rows, ids, vectors, _bridge, ref, walks = corpus[metric]
    s = build_three_segments(ctx, metric, rows, ids, FORMS[form])
    plain = plain_scores(s, vectors, ids)
    compounds = COMPOUNDS + ([] if form == "wave" else COMPOUNDS_W8)
    n_first = n_later = n_open = 0
    for mode, lam, k, pool in plan(form):
        got = compound(s, vectors, compounds, k, mode, lam, pool)
        for i, c in enumerate(compounds):
            want = model_walk(ref, walks, c, mode, lam, k, pool)
            check(got, want, i, k)
            check_parts_against_plain(got, plain, c, i)
            n_first += want.exact and want.examined <= 128
            n_later += want.exact and want.examined > 128
            n_open += not want.exact
            if got[6][i]:  # a 1 is a proof: the rows are those of the whole corpus
                check(got, model_brute(ref, walks, c, mode, lam, k), i, k, rows_only=True)
    print(form, metric, "first pass", n_first, "later", n_later, "at the pool", n_open)
    assert n_first > 30 and n_later > 15 and n_open > 30
    if form == "wave":  # eight wanted vectors do not fit the wave kernel's pass of four: refused before any launch
        with pytest.raises(pa.PcvError) as err:
            compound(s, vectors, COMPOUNDS[:2] + COMPOUNDS_W8[:1], 10, ALL, 0.5, 128)
        assert err.value.status == 3 and "compound 2 has 8 wanted vectors" in str(err.value) and "takes 4 queries" in str(err.value)
    # the default pool is search_boosted's rule
    got = compound(s, vectors, compounds, 10, ALL, 0.5, None)
    for i, c in enumerate(compounds):
        check(got, model_walk(ref, walks, c, ALL, 0.5, 10, cr.default_pool(10)), i, 10)
    s.close()


# ---- 2. identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_identities(ctx, corpus, metric):
    rows, ids, vectors, _bridge, _ref, _walks = corpus[metric]
    s = build_three_segments(ctx, metric, rows, ids, FORMS["mfma_int8"])
    singles = [((v,), ()) for v in range(16)]
    for k, pool in ((1, 1), (10, 10), (10, 128), (127, 128), (128, 4096)):
        p_ids, p_scores, p_counts = s.search_vectors(None, k, vectors[:16])
        for mode in (ALL, ANY):
            # W = 1, A = 0: the plain search, ids and score bits
            got = compound(s, vectors, singles, k, mode, 1.0, pool)
            np.testing.assert_array_equal(got[0], p_ids)
            np.testing.assert_array_equal(bits32(got[2][:, :, 0]), bits32(p_scores))
            np.testing.assert_array_equal(got[4], p_counts)
            assert np.isnan(got[2][:, :, 1:]).all() and (got[3] == 0.0).all()
            assert bool(got[6].all()) == bool(got[6].any()) == (pool > k)  # (k entries of k walked: m_k == T, which is no proof)
            # the same vector twice: the same rows, none twice
            twice = compound(s, vectors, [((v, v), ()) for v in range(16)], k, mode, 1.0, pool)
            np.testing.assert_array_equal(twice[0], p_ids)
            np.testing.assert_array_equal(bits64(twice[1]), bits64(got[1]))
            np.testing.assert_array_equal(bits32(twice[2][:, :, 1]), bits32(p_scores))
            for i in range(16):
                assert len(set(twice[0][i].tolist())) == k
    # ANY over [q1, q2]: the merge of the two plain lists under the better score, each row once
    n = ids.shape[0]
    f_ids, f_scores, _c = s.search_vectors(None, n, vectors[:16])
    # (the dot metric reports max(0, 1 - c / dim), which is 0 for every good row of a noisy anchor: there only the Gaussian pairs)
    pairs = [((a, a + 1), ()) for a in range(8 if metric == "dot" else 0, 16, 2)]
    got = compound(s, vectors, pairs, 10, ANY, 1.0, 128)
    assert got[6].all() and (got[5] == 128).all()
    for i, (w, _a) in enumerate(pairs):
        best = {}
        for v in w:
            for item, sc in zip(f_ids[v].tolist(), f_scores[v].tolist()):
                better = (sc < best[item]) if metric == "dot" and item in best else (item not in best or sc > best[item])
                if better:
                    best[item] = sc
        merged = sorted(best, key=lambda item: best[item] if metric == "dot" else -best[item])[:10]
        assert got[0][i].tolist() == merged
        assert len(set(got[0][i].tolist())) == 10
    # a weight of 0 with avoided vectors present: the same compound without them
    with_avoid = [(w, (16, 17)) for w, _a in pairs]
    for mode in (ALL, ANY):
        a = compound(s, vectors, with_avoid, 10, mode, 0.0, 300)
        b = compound(s, vectors, pairs, 10, mode, 0.0, 300)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint8) if x.dtype.kind == "f" else x, y.view(np.uint8) if y.dtype.kind == "f" else y)
        assert (a[3] == 0.0).all()
    s.close()


# ---- 3. groups never split a compound ----------------------------------------------------------------------------------------------
def many_compounds(n):
    """n compounds of four wanted vectors each, with an avoided vector for every third; every fourth is a pair of planted neighbours
    twice over, which the bridge rows certify in the first pass while the others of its group walk on"""
    out = []
    for i in range(n):
        a = 2 * ((i // 4) % 4)
        want = (a, a + 1, a, a + 1) if i % 4 == 0 else (i % 24, (i + 1) % 24, (i + 5) % 24, (i + 11) % 24)
        out.append((want, ((i + 3) % 24,) if i % 3 == 0 else ()))
    return out


@pytest.mark.parametrize("form,compounds", [("wave", [((0, 1, 2), ()), ((8, 9), (16,)), ((4, 5), ())]), ("mfma_f32", many_compounds(40)),
                                            ("mfma_int8", many_compounds(70))], ids=["wave_3_2_2", "f32_40x4", "int8_70x4"])
def test_groups(ctx, corpus, form, compounds):
    rows, ids, vectors, _bridge, ref, walks = corpus["cosine"]
    assert all(len(w) == 4 for w, _a in compounds) or form == "wave"
    s = build_three_segments(ctx, "cosine", rows, ids, FORMS[form])
    k, pool = 10, 300
    for mode in (ALL, ANY):
        got = compound(s, vectors, compounds, k, mode, 0.5, pool)
        model = [model_walk(ref, walks, c, mode, 0.5, k, pool) for c in compounds]
        for i in range(len(compounds)):  # (a finished compound's rows did not change while the others of its group walked on)
            check(got, model[i], i, k)
        assert mode == ANY or len({w.examined for w in model}) > 1  # (ALL: some of a group finish while others walk on)
        for i in sorted({0, 1, len(compounds) // 2, len(compounds) - 1}):  # ... as in a call of its own
            one = compound(s, vectors, compounds[i : i + 1], k, mode, 0.5, pool)
            for a, b in zip(got, one):
                np.testing.assert_array_equal(a[i : i + 1].view(np.uint8) if a.dtype.kind == "f" else a[i : i + 1], b.view(np.uint8) if b.dtype.kind == "f" else b)
    s.close()


# ---- 4. what is selected ----------------------------------------------------------------------------------------------------------
def test_selection(ctx, corpus):
    rows, ids, vectors, bridge_ids, ref, walks = corpus["cosine"]
    s = build_three_segments(ctx, "cosine", rows, ids, FORMS["mfma_int8"])
    n = ids.shape[0]
    compounds = COMPOUNDS[:6]
    k, pool = 10, 300

    def run(searcher, allowed, tag, sources=None):
        for mode in (ALL, ANY):
            got = compound(searcher, vectors, compounds, k, mode, 0.5, pool, sources)
            for i, c in enumerate(compounds):
                check(got, model_walk(ref, walks, c, mode, 0.5, k, pool, allowed, tag), i, k)
        return got

    # the source filter
    run(s, np.arange(SPLIT[1], n), "source2", [2])
    # hidden bridge rows are not returned and do not count as examined
    before = compound(s, vectors, [COMPOUNDS[1]], k, ALL, 0.5, 4096)
    assert set(before[0][0].tolist()) <= set(np.concatenate(bridge_ids).tolist())
    hidden = bridge_ids[0]
    s.hide_items(hidden)
    shown = np.nonzero(~np.isin(ids, hidden))[0]
    run(s, shown, "hidden")
    after = compound(s, vectors, [COMPOUNDS[1]], k, ALL, 0.5, 4096)
    assert not np.isin(after[0], hidden).any() and after[0][0].tolist() != before[0][0].tolist()
    want = ref.walk(COMPOUNDS[1][0], (), ALL, 0.5, k, 4096, shown)
    check(after, want, 0, k)
    # a view walks its own rows
    half = ids[::2]
    v = s.view(half)
    run(v, np.nonzero(np.isin(ids, half) & ~np.isin(ids, hidden))[0], "view")
    v.close()
    s.unhide_items(hidden)
    # an empty selection: the blank answer, exact
    got = compound(s, vectors, compounds, k, ALL, 0.5, pool, [])
    assert (got[4] == 0).all() and (got[5] == 0).all() and got[6].all()
    assert (got[0] == -1).all() and np.isnan(got[1]).all() and np.isnan(got[2]).all() and np.isnan(got[3]).all()
    # the like-items form against the vector form, with the vectors from like_queries
    items = [int(ids[x]) for x in (5, 700, 1500, 2900, 40)]
    groups = [[items[0]], [items[1], items[2]], [items[3]], [items[4]]]
    weights = [[1.0], [0.5, 2.0], [1.0], [1.0]]
    vec, found, _members = s.like_queries(groups, weights)
    assert found.all()
    wants_like = [[[items[0]], [(items[1], 0.5), (items[2], 2.0)]], [[items[3]]]]
    avoids_like = [[[items[4]]], []]
    for mode in ("all", "any"):
        a = s.search_compound_like_items(None, k, wants_like, avoids_like, mode, 0.5, pool, exclude_examples=False)
        b = s.search_compound(None, k, [vec[:2], vec[2:3]], [vec[3:4], np.zeros((0, D), np.float32)], mode, 0.5, pool)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint8) if x.dtype.kind == "f" else x, y.view(np.uint8) if y.dtype.kind == "f" else y)
        assert items[3] == a[0][1, 0]  # (one example, W = 1: the item itself comes first)
        # exclude_examples: the wanted examples are left out, the rest is the same list
        e = s.search_compound_like_items(None, k, wants_like, avoids_like, mode, 0.5, pool, exclude_examples=True)
        wide = s.search_compound(None, k + 3, [vec[:2], vec[2:3]], [vec[3:4], np.zeros((0, D), np.float32)], mode, 0.5, pool)
        for i, own in enumerate(([items[0], items[1], items[2]], [items[3]])):
            rest = [x for x in wide[0][i].tolist() if x not in own][:k]
            assert e[0][i].tolist() == rest and not set(own) & set(e[0][i].tolist()) and e[4][i] == k
    with pytest.raises(pa.PcvError) as err:  # a part none of whose examples is stored is a zero vector: no cosine
        s.search_compound_like_items(None, k, [[[-12345]]], None)
    assert err.value.status == 1 and "no cosine is defined" in str(err.value)
    s.close()


def test_bad_vectors_and_an_unfinalized_searcher(ctx):
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((40, 32)).astype(np.float32)
    s = pa.Searcher(ctx, 32, "cosine")
    s.add_rows(1, rows, np.arange(40))
    with pytest.raises(pa.PcvError) as plain:
        s.search_vectors(None, 5, rows[:1])
    with pytest.raises(pa.PcvError) as comp:
        s.search_compound(None, 5, [rows[:2]])
    assert comp.value.status == plain.value.status
    assert str(comp.value).endswith("search_compound: rows were added or cleared without pcv_searcher_finalize")
    s.finalize()
    got = s.search_compound(None, 5, [rows[:2]], [rows[2:3]], "any", 0.5)
    assert got[4][0] == 5 and got[6][0] and got[5][0] == 40
    for bad in (np.nan, np.inf, -np.inf):
        v = rows[:2].copy()
        v[1, 7] = bad
        for wants, avoids, side in (([v], None, "wanted"), ([rows[:1]], [v], "avoided")):
            with pytest.raises(pa.PcvError) as err:
                s.search_compound(None, 5, wants, avoids)
            assert err.value.status == 1 and "value 7 of %s vector 1 is not finite" % side in str(err.value)
    zero = np.zeros((1, 32), dtype=np.float32)
    tiny = np.full((1, 32), 1e-30, dtype=np.float32)
    for v in (zero, tiny):
        for wants, avoids, side in (([v], None, "wanted"), ([rows[:1]], [v], "avoided")):
            with pytest.raises(pa.PcvError) as err:
                s.search_compound(None, 5, wants, avoids)
            assert err.value.status == 1 and "%s vector 0 has squared norm" % side in str(err.value)
    s.close()


# ---- 5. the padded last piece, and vectors too wide for the LDS ----------------------------------------------------------------------
def test_padded_width(ctx, oracle):
    dim = 100
    rows, ids, anchors, _bridge = cr.bridged_corpus(planted_corpus, "cosine", dim=dim)
    vectors = cr.compound_vectors(planted_queries, "cosine", anchors, dim=dim)
    ref = cr.CompoundReference(oracle, vectors, rows, ids, "cosine")
    s = build_three_segments(ctx, "cosine", rows, ids, FORMS["mfma_int8"], dim=dim)
    plain = plain_scores(s, vectors, ids)
    compounds = COMPOUNDS[1:4] + COMPOUNDS_W8[2:]
    for mode in (ALL, ANY):
        for k, pool in ((10, 128), (128, 300), (10, 4096)):
            wants = [vectors[list(w)] for w, _a in compounds]
            avoids = [vectors[list(a)] for _w, a in compounds]
            got = s.search_compound(None, k, wants, avoids, MODES[mode], 0.5, pool)
            for i, c in enumerate(compounds):
                check(got, ref.walk(c[0], c[1], mode, 0.5, k, pool), i, k)
                check_parts_against_plain(got, plain, c, i)
    s.close()


def test_vectors_read_from_global_memory(ctx, oracle):
    """16 vectors of 2112 features are 132 KB: more than the select step stages in LDS"""
    dim, n = 2112, 320
    rng = np.random.default_rng(2112)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    ids = (rng.permutation(n) * 5 + 77).astype(np.int64)
    vectors = rng.standard_normal((24, dim)).astype(np.float32)
    vectors[:8] += rows[:8]
    ref = cr.CompoundReference(oracle, vectors, rows, ids, "cosine")
    s = build(ctx, dim, "cosine", [(1, rows[:200], ids[:200]), (2, rows[200:], ids[200:])], screen="off", kernel="mfma")
    plain = plain_scores(s, vectors, ids)
    compounds = [COMPOUNDS_W8[2], COMPOUNDS[8], COMPOUNDS[1]]
    for mode in (ALL, ANY):
        for k, pool in ((10, 128), (10, 300), (128, 4096)):
            got = compound(s, vectors, compounds, k, mode, 0.5, pool)
            for i, c in enumerate(compounds):
                check(got, ref.walk(c[0], c[1], mode, 0.5, k, pool), i, k)
                check_parts_against_plain(got, plain, c, i)
    s.close()


# ---- 6. the C++ mirror -----------------------------------------------------------------------------------------------------------
def hashed_rows(n, dim):
    """the rows of tests/cpp/compound_mirror_test.cpp"""
    i = np.arange(n, dtype=np.uint64)[:, None]
    j = np.arange(dim, dtype=np.uint64)[None, :]
    m = np.uint64(0xFFFFFFFF)
    h = (i * np.uint64(2654435761) + j * np.uint64(40503) + np.uint64(12345)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & m
    h ^= h >> np.uint64(13)
    return ((h >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0) - np.float32(0.5)).astype(np.float32)


def test_cpp_mirror_compound_program(ctx):
    src = os.path.join(ROOT, "tests", "cpp", "compound_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "compound_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "compound_mirror_test: ok" in r.stdout
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
    got = s.search_compound([1, 2], 10, [rows[[77, 78]]], [rows[[79]]], "all", 0.5, 300)
    assert got[4][0] == 10
    ours = [[int(got[0][0, j]), int(bits64(got[1][0, j : j + 1])[0]), int(bits32(got[2][0, j, 0:1])[0]), int(bits32(got[2][0, j, 1:2])[0]),
             int(bits64(got[3][0, j : j + 1])[0])] for j in range(10)]
    assert printed == ours and exact == [int(got[6][0])]
    s.close()
