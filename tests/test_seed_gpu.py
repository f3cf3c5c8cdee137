"""GPU: the threshold a top-k pass starts from — the four seed kernels, seed_threshold_key / is_seed_block and set_guess —
against the float64 model of tests/seed_ref.py.

test_screens_gpu.py pins every screen's survivor counts under a range pass, whose thresholds nothing raises.  Here the pass is a
top-k pass on a planted corpus (seed_ref.Pinned): the k best rows of every query are seed rows, one in each of the k seed groups,
and the guess is off, so min(slots) is the final k-th best score from the seed on, no offer of the scan succeeds, and the counts
the pass reports are a function of the seed alone — held to the model's bracket from both sides.  A seed that is too loose (a slot
never filled, a group lost, a block skipped) lets thousands of rows more through; one that is too tight loses planted hits.
The guess cases (seed_ref.Guess) hold the counts to the high end of the bracket at the model's guess, from one side: the scan
raises tau above the guess at a pace nobody can model.  The exactness edges compare hits and scores with the oracle where the
seed's indexing can go wrong: short first segments, rows stored twice, hidden and scoreless seed rows, a source filter, k = 1,
128 and 300.  tests/test_seed_cpu.py checks the conditions on the inputs that all of this rests on."""
from collections import namedtuple

import numpy as np
import pytest

import perceive_amd as pa
import seed_ref as sd
from seed_ref import with_parts
from six_ref import reported

pytestmark = pytest.mark.gpu

COPY = {"int8": ("int8", 2, 8), "bf16": ("bf16", 1, 0), "f32": ("off", 0, 0), "wave": ("off", 0, 0)}  # set_screening_copy, screening_copy, screen_bits
NAMES = {"coarse": "coarse_survivors", "mid": "mid_survivors", "candidates": "candidates"}
MET = {"cosine": 0, "dot": 1}


def build(ctx, D, metric, flags, screen, mid, segments, capacity=4096):
    """a searcher with one segment per entry of `segments` ([(rows, ids)]; sources 1, 2, ...)"""
    s = pa.Searcher(ctx, D, metric)
    s.set_tuning(flags)
    s.set_screening_copy(COPY[screen][0])
    s.set_mid_copy(mid)
    if screen in ("f32", "bf16"):
        s.set_kernel("mfma")  # (AUTO takes the wave kernel for up to four queries without a copy)
    s.set_candidate_capacity(capacity)
    for i, (rows, ids) in enumerate(segments):
        s.add_rows(i + 1, rows, ids)
        s.finalize()
    assert s.num_segments == len(segments)
    return s


def check_hits(oracle, got, queries, corpus, k, metric, keep=None):
    """hits and scores against oracle.topk over corpus[keep] (default: all rows); ids are positions in `corpus`"""
    ids, scores, counts = got
    keep = np.arange(len(corpus)) if keep is None else np.asarray(keep)
    opos, osc, ocnt = oracle.topk(queries, corpus[keep], k, metric=MET[metric])
    want = np.where(opos >= 0, keep[np.maximum(opos, 0)], -1)
    np.testing.assert_array_equal(counts, ocnt)
    np.testing.assert_array_equal(ids, want)
    for b in range(len(queries)):
        np.testing.assert_allclose(scores[b, : ocnt[b]], reported(osc[b, : ocnt[b]], metric, corpus.shape[1]), rtol=0, atol=1e-7)
    return want


# ---- pinned cases: the counts are a function of the seed alone ------------------------------------------------------------------------------
PINNED_IDS = [f"{s.form}-{s.D}d-B{s.B}-k{s.k}-{s.rows}" for s in sd.PINNED]


@pytest.mark.parametrize("metric", sd.METRICS)
@pytest.mark.parametrize("shape", sd.PINNED, ids=PINNED_IDS)
def test_pinned_counts(ctx, oracle, shape, metric):
    c = sd.Pinned.get(shape, metric)
    assert sd.form_of(shape) == shape.form and sd.seed_plan(shape.rows, shape.flags) == c.plan  # (no statistic reports either)
    want = c.bracket()
    s = build(ctx, shape.D, metric, shape.flags, shape.screen, shape.mid, [(c.corpus, np.arange(shape.rows, dtype=np.int64))])
    try:
        got = s.search_vectors(None, shape.k, c.queries)
        st = s.last_stats()
        print(f"D={shape.D} {metric} B={shape.B} k={shape.k} seed {shape.form} plan={c.plan} {sd.scan_of(shape)}: "
              + ", ".join(f"{n} {st[NAMES[n]]} (model {lo} .. {hi})" for n, (lo, hi) in want.items()))
        assert st["scan_launches"] == 1 and st["overflow_reruns"] == 0 and st["speculation_reruns"] == 0, st
        assert st["screening_copy"] == COPY[shape.screen][1] and st["screen_bits"] == COPY[shape.screen][2]
        assert st["mid_copy"] == (1 if shape.mid == "on" else 0)
        hits = check_hits(oracle, got, c.queries, c.corpus, shape.k, metric)
        for b in range(shape.B):
            assert set(hits[b].tolist()) == set(c.planted[c.cluster[b]].tolist())
        for n, (lo, hi) in want.items():
            assert lo <= st[NAMES[n]] <= hi, (n, st[NAMES[n]], lo, hi)
        if shape.mid != "on":
            assert st["mid_survivors"] == 0
    finally:
        s.close()


# ---- guess cases: the counts from one side ------------------------------------------------------------------------------------------------
GUESS_IDS = [f"{s.screen}-{s.D}d-B{s.B}-k{s.k}" for s in sd.GUESS]


@pytest.mark.parametrize("metric", sd.METRICS)
@pytest.mark.parametrize("shape", sd.GUESS, ids=GUESS_IDS)
def test_guess_counts(ctx, oracle, shape, metric):
    """a fresh searcher without the learned part (kFlagNoLearnedGuess): the guess is the rank-th largest seed slot, raised by
    quantize_queries_kernel (int8 scan) or set_guess_kernel (bf16 copy); it holds, and every count is at most the high end of the
    bracket at the model's guess (k = 2: no guess at this size, the bound is the one at min(slots))"""
    c = sd.Guess.get(shape, metric)
    high = c.high(shape)
    q = c.queries[: shape.B]
    s = build(ctx, shape.D, metric, shape.flags, shape.screen, "off", [(c.corpus, np.arange(shape.rows, dtype=np.int64))], capacity=1 << 15)
    try:
        got = s.search_vectors(None, shape.k, q)
        st = s.last_stats()
        print(f"D={shape.D} {metric} B={shape.B} k={shape.k} rank={c.rank} {sd.scan_of(shape)}: "
              + ", ".join(f"{n} {st[NAMES[n]]} (model <= {hi}; without the guess >= {c.low_without(shape)[n]})" for n, hi in high.items()))
        assert st["speculation_reruns"] == 0 and st["overflow_reruns"] == 0 and st["scan_launches"] == 1, st
        assert st["screening_copy"] == COPY[shape.screen][1]
        hits = check_hits(oracle, got, q, c.corpus, shape.k, metric)
        for b in range(shape.B):
            assert set(hits[b].tolist()) == set(c.planted[b].tolist())
        for n, hi in high.items():
            assert st[NAMES[n]] <= hi, (n, st[NAMES[n]], hi)
    finally:
        s.close()


# ---- exactness edges ----------------------------------------------------------------------------------------------------------------------
# one MFMA-seed shape, one valu8 shape, one valu1 shape; one seed part unless a case says otherwise; the guess as a search has it
Edge = namedtuple("Edge", "form D B screen flags")
EDGES = [Edge("mfma", 128, 8, "int8", sd.N8), Edge("valu8", 1536, 5, "f32", 0), Edge("valu1", 2048, 7, "f32", 0)]
EDGE_IDS = [f"{e.form}-{e.D}d-B{e.B}" for e in EDGES]
N_EDGE = 3007


def edge_inputs(edge, metric, salt, n=N_EDGE):
    rng = np.random.default_rng(9900 + edge.D + 17 * salt + MET[metric])
    x = sd._background(rng, n, edge.D, metric).astype(np.float32)
    q = rng.standard_normal((edge.B, edge.D))
    return rng, x, q, (q * rng.uniform(0.5, 2.0, (edge.B, 1))).astype(np.float32)


def near_copies(rng, q, levels, metric):
    """graded near-copies of the direction q: rows at cosines `levels` with it"""
    rows = sd._near(rng, sd._unit(q), np.asarray(levels, dtype=np.float64))
    return (rows * (sd.RADIUS if metric == "dot" else rng.uniform(0.5, 2.0, (len(levels), 1)))).astype(np.float32)


def open_edge(ctx, edge, metric, segments, k, flags=with_parts(1)):
    """-> (a searcher of one source per segment whose ids are the rows' positions, the segments as one corpus)"""
    assert sd.seed_form(edge.B, sd.padded(edge.D), min(k, sd.MAX_K), edge.flags | flags) == edge.form
    ids, at = [], 0
    for seg in segments:
        ids.append(np.arange(at, at + len(seg), dtype=np.int64))
        at += len(seg)
    return build(ctx, edge.D, metric, edge.flags | flags, edge.screen, "off", list(zip(segments, ids))), np.concatenate(segments)


@pytest.mark.parametrize("metric", sd.METRICS)
@pytest.mark.parametrize("n0", [1, 31, 33, 401])
@pytest.mark.parametrize("edge", EDGES, ids=EDGE_IDS)
def test_short_first_segment(ctx, oracle, edge, n0, metric):
    """segment 0 of 1, 31, 33 and 401 rows in front of a segment of 3 007: fewer seed rows than k, a partial last seed block, and
    at 401 rows, under the default parts, 13 seed blocks — a multiple of neither 4 nor 8: the MFMA seed's fourth workgroup has
    one live wave of four, the VALU seed's second part five live blocks of eight, and block 12 holds 17 rows.  Up to seven of
    each query's 14 planted rows are seed rows of segment 0, the others lie in the large segment, which has no seed rows at all."""
    k = 10
    rng, big, q, queries = edge_inputs(edge, metric, n0)
    small = sd._background(rng, n0, edge.D, metric).astype(np.float32)
    flags = 0 if n0 == 401 else with_parts(1)
    plan = sd.seed_plan(n0, flags)
    _, srow = sd.seed_sample(n0, plan)
    assert plan == {1: (1, 0), 31: (1, 0), 33: (2, 0), 401: (13, 0)}[n0] and len(srow) == n0
    spots = rng.permutation(N_EDGE)[: edge.B * 14].reshape(edge.B, 14)
    front = rng.permutation(srow)
    for b in range(edge.B):
        rows = near_copies(rng, q[b], np.linspace(0.9, 0.5, 14), metric)
        mine = front[b::edge.B][:7]  # this query's seed rows: every B-th of the shuffled sample
        order = rng.permutation(14)
        small[mine] = rows[order[: len(mine)]]
        big[spots[b, len(mine):]] = rows[order[len(mine):]]
    s, corpus = open_edge(ctx, edge, metric, [small, big], k, flags=flags)
    try:
        check_hits(oracle, s.search_vectors(None, k, queries), queries, corpus, k, metric)
        assert s.last_stats()["scan_launches"] == 1 + s.last_stats()["speculation_reruns"] + s.last_stats()["overflow_reruns"]
    finally:
        s.close()


@pytest.mark.parametrize("metric", sd.METRICS)
@pytest.mark.parametrize("placement", ["next_block", "same_group", "different_groups", "outside"])
@pytest.mark.parametrize("edge", EDGES, ids=EDGE_IDS)
def test_rows_stored_twice(ctx, oracle, edge, placement, metric):
    """every one of a query's ten best rows is stored twice; a search for 20 returns both copies, the lower position first.
    One copy in a seed block and one in the block after it (is_seed_block must tell them apart); both in one seed group (one
    slot for two equal scores: min(slots) must not count the row twice); in different groups; both outside the seed."""
    k, pairs = 20, 10
    rng, x, q, queries = edge_inputs(edge, metric, len(placement))
    plan = sd.seed_plan(N_EDGE, with_parts(1))
    sample, srow = sd.seed_sample(N_EDGE, plan)
    row_of = dict(zip(sample.tolist(), srow.tolist()))
    outside = np.setdiff1d(np.arange(N_EDGE - 64), np.concatenate([srow, srow + 32]))
    where = []
    for p in range(edge.B * pairs):
        if placement == "next_block":
            where.append((row_of[3 * p], row_of[3 * p] + 32))
        elif placement == "same_group":
            a = (p // k) * 2 * k + p % k
            where.append((row_of[a], row_of[a + k]))
        elif placement == "different_groups":
            where.append((row_of[2 * p], row_of[2 * p + 1]))
        else:
            where.append((int(outside[2 * p]), int(outside[2 * p + 1])))
    where = np.array(where)
    assert len(np.unique(where)) == where.size and (where[:, 0] < where[:, 1]).all()
    in_seed = np.isin(where, srow)
    assert (in_seed == {"next_block": [True, False], "outside": [False, False]}.get(placement, [True, True])).all()
    if placement == "same_group":
        pos = {r: s_ for s_, r in row_of.items()}
        assert all(pos[a] % k == pos[b] % k for a, b in where)
    for b in range(edge.B):
        rows = near_copies(rng, q[b], np.linspace(0.9, 0.6, pairs), metric)
        x[where[b * pairs:(b + 1) * pairs, 0]] = rows
        x[where[b * pairs:(b + 1) * pairs, 1]] = rows
    s, corpus = open_edge(ctx, edge, metric, [x], k)
    try:
        got = s.search_vectors(None, k, queries)
        hits = check_hits(oracle, got, queries, corpus, k, metric)
        for b in range(edge.B):
            np.testing.assert_array_equal(hits[b].reshape(pairs, 2), where[b * pairs:(b + 1) * pairs])
            np.testing.assert_array_equal(got[1][b, 0::2], got[1][b, 1::2])
    finally:
        s.close()


@pytest.mark.parametrize("metric", sd.METRICS)
@pytest.mark.parametrize("edge", EDGES, ids=EDGE_IDS)
def test_seed_rows_without_a_score(ctx, oracle, edge, metric):
    """each query's three best rows are seed rows hidden with hide_items; all-zero rows and rows with a NaN or an inf sit in
    seed blocks as well: none of them may fill a slot, and the hits are the oracle's over the rows that are left"""
    k = 10
    rng, x, q, queries = edge_inputs(edge, metric, 5)
    _, srow = sd.seed_sample(N_EDGE, sd.seed_plan(N_EDGE, with_parts(1)))
    front = rng.permutation(srow)
    hidden = []
    for b in range(edge.B):
        mine = front[b * 14:(b + 1) * 14]
        x[mine] = near_copies(rng, q[b], np.linspace(0.95, 0.5, 14), metric)
        hidden += mine[:3].tolist()
    rest = front[edge.B * 14:]
    x[rest[0:4]] = 0.0
    x[rest[4], 7] = np.nan
    x[rest[5]] = near_copies(rng, q[0], [0.99], metric)[0]
    x[rest[5], 3] = np.inf
    x[rest[6]] = near_copies(rng, q[1], [0.99], metric)[0]
    x[rest[6], edge.D - 1] = -np.inf
    s, corpus = open_edge(ctx, edge, metric, [x], k)
    try:
        assert s.hide_items(np.array(hidden, dtype=np.int64)) == len(hidden)
        keep = np.setdiff1d(np.arange(N_EDGE), np.concatenate([hidden, rest[4:7]]))
        hits = check_hits(oracle, s.search_vectors(None, k, queries), queries, corpus, k, metric, keep=keep)
        for b in range(edge.B):
            assert set(hits[b].tolist()) == set(front[b * 14 + 3: b * 14 + 13].tolist())
    finally:
        s.close()


@pytest.mark.parametrize("metric", sd.METRICS)
@pytest.mark.parametrize("edge", EDGES, ids=EDGE_IDS)
def test_source_filter_moves_the_first_segment(ctx, oracle, edge, metric):
    """two sources of 3 007 rows, the search takes the second: the pass's first segment is the searcher's second.  Each query's
    hits are seed rows of the selected segment; the same rows of the unselected one hold better near-copies still, which are no
    hits and must not fill a slot"""
    k = 10
    rng, x2, q, queries = edge_inputs(edge, metric, 6)
    x1 = sd._background(rng, N_EDGE, edge.D, metric).astype(np.float32)
    _, srow = sd.seed_sample(N_EDGE, sd.seed_plan(N_EDGE, with_parts(1)))
    front = rng.permutation(srow)
    for b in range(edge.B):
        mine = front[b * 14:(b + 1) * 14]
        x2[mine] = near_copies(rng, q[b], np.linspace(0.8, 0.45, 14), metric)
        x1[mine] = near_copies(rng, q[b], np.linspace(0.99, 0.9, 14), metric)
    s, corpus = open_edge(ctx, edge, metric, [x1, x2], k)
    try:
        keep = np.arange(N_EDGE, 2 * N_EDGE)
        hits = check_hits(oracle, s.search_vectors([2], k, queries), queries, corpus, k, metric, keep=keep)
        for b in range(edge.B):
            assert set(hits[b].tolist()) == set((N_EDGE + front[b * 14: b * 14 + 10]).tolist())
        check_hits(oracle, s.search_vectors([1], k, queries), queries, corpus, k, metric, keep=np.arange(N_EDGE))
    finally:
        s.close()


@pytest.mark.parametrize("metric", sd.METRICS)
@pytest.mark.parametrize("k", [1, 128, 300])
@pytest.mark.parametrize("edge", EDGES, ids=EDGE_IDS)
def test_one_result_and_many(ctx, oracle, edge, k, metric):
    """k = 1 (one slot, one group), k = 128 (as many slots as there are) and num_results = 300: three passes, the second and third
    under ceilings, so that ceil_class runs in the seed kernel.  Two seed parts: 16 seed blocks, every fourth of 94; the 320 best
    rows of every query — the queries are near-copies of one direction — are seed rows"""
    flags = with_parts(2)
    rng, x, _, _ = edge_inputs(edge, metric, 7)
    centre = sd._unit(rng.standard_normal(edge.D))
    queries = ((centre[None, :] + 0.01 * sd._unit(rng.standard_normal((edge.B, edge.D)))) * rng.uniform(0.5, 2.0, (edge.B, 1))).astype(np.float32)
    plan = sd.seed_plan(N_EDGE, flags)
    _, srow = sd.seed_sample(N_EDGE, plan)
    assert plan == (16, 2) and len(srow) == 512
    planted = rng.permutation(srow)[:320]
    x[planted] = near_copies(rng, centre, np.linspace(0.95, 0.5, 320), metric)
    s, corpus = open_edge(ctx, edge, metric, [x], k, flags=flags)
    try:
        hits = check_hits(oracle, s.search_vectors(None, k, queries), queries, corpus, k, metric)
        assert np.isin(hits, planted).all()
        assert s.last_stats()["scan_launches"] >= (k + sd.MAX_K - 1) // sd.MAX_K
    finally:
        s.close()
