"""GPU: the candidate counts of the row-pair screens — find_duplicates, density_clusters, assign, neighbors, linkage_tree,
reach_tree — against the brackets of the float64 model of pairs_ref.py, from above as well as from below.  The exact f64 step hides
every screen error that only adds candidates; the counts do not.

Every test first compares the call's result with the reference the screen's own tests use (the check functions of *_ref.py), then
asserts lo <= count <= hi and the stats that show which form ran: the tile, the sample, the spans, the label tiles, the reruns,
the rounds.  The runs are pairs_ref.RUNS, the list test_pairs_cpu.py holds to its width caps: 3 007 rows (94 blocks, a last block of
31 rows, a partial last tile) at every chunk count and tile size of pair_screen.h, 12 320 rows (a second span, a sampled bound
pass), eight segments in three sources, rows that take no part and wild rows, lists that outgrow their first room.  No count of a
device is written down here: the brackets come from the inputs alone."""
import numpy as np
import pytest

import perceive_amd as pa
import assign_ref
import density_ref
import duplicates_ref
import linkage_ref
import neighbors_ref
import pairs_ref as pr
import reach_ref

pytestmark = pytest.mark.gpu

MAX_VERIFIED_ROWS = 4000  # above it the trees' verifier takes minutes: the edges are compared with the model's exact tree instead


def runs_of(screen):
    rs = [r for r in pr.RUNS if r.screen == screen]
    return pytest.mark.parametrize("r", rs, ids=[pr.run_id(r) for r in rs])


def open_searcher(ctx, r, metric="cosine"):
    """-> (searcher, source list of the call, rows, ids, part of the selected rows in the order of their global positions)"""
    md = pr.made(r.key)
    s = pa.Searcher(ctx, md.rows.shape[1], metric)
    for sid, lo, hi in md.pieces:
        s.reserve(sid, hi - lo)
        s.add_rows(sid, md.rows[lo:hi], md.ids[lo:hi])
        s.finalize()
    assert s.num_rows == len(md.rows) and s.num_segments == len(md.pieces)
    if md.hidden.any():
        assert s.hide_items(md.ids[md.hidden]) == int(md.hidden.sum())
    sel = np.concatenate(pr.selected(md, r.select))
    return s, (None if r.select is None else list(r.select)), np.ascontiguousarray(md.rows[sel]), md.ids[sel], ~md.hidden[sel]


def held(r, name, count, lo, hi):
    print("PAIRS %s %s: device %d, model %d .. %d" % (pr.run_id(r), name, count, lo, hi))
    assert lo <= count <= hi, (pr.run_id(r), name, count, lo, hi)


@runs_of("join")
def test_join(ctx, oracle, r):
    s, src, rows, ids, part = open_searcher(ctx, r)
    got = s.find_duplicates(src, r.args[0])
    st = s.last_duplicate_stats()
    s.close()
    duplicates_ref.check(got, duplicates_ref.reference(oracle, rows, ids, r.args[0], np.nonzero(part)[0]))
    c = pr.model(r.key, r.select).c
    assert st["rows"] == len(rows) and st["tile_rows"] == c.tile and st["reruns"] == (1 if r.grows else 0)
    assert (pr.join_spans(c.TB) > 1) == (r.key == "big64")
    held(r, "candidates", st["candidates"], *pr.bracket(r))


@runs_of("density")
def test_density(ctx, oracle, r):
    s, src, rows, ids, part = open_searcher(ctx, r)
    got = s.density_clusters(src, *r.args)
    st = s.last_density_stats()
    s.close()
    density_ref.check(got, density_ref.reference(oracle, rows, ids, r.args[0], r.args[1], part), st)
    assert st["tile_rows"] == pr.model(r.key, r.select).c.tile and st["reruns"] == (1 if r.grows else 0)
    for name, (lo, hi) in pr.bracket(r).items():
        held(r, name, st[name], lo, hi)


@runs_of("assign")
def test_assign(ctx, oracle, r):
    lab, metric = pr.assign_labels(r)
    s, src, rows, ids, part = open_searcher(ctx, r, metric)
    got = s.assign(src, lab)
    st = s.last_assign_stats()
    s.close()
    assign_ref.check_assign(got, assign_ref.assign_reference(oracle, rows, lab, metric, part), ids)
    tile = pr.model(r.key, r.select).c.tile
    assert st["rows"] == len(rows) and st["tile_labels"] == tile and st["label_tiles"] == -(-len(lab) // tile)
    assert st["reruns"] == (1 if r.grows else 0)
    held(r, "candidates", st["candidates"], *pr.bracket(r))


@runs_of("neighbors")
def test_neighbors(ctx, oracle, r):
    k = r.args[0]
    s, src, rows, ids, part = open_searcher(ctx, r)
    got = s.neighbors(src, k)
    st = s.last_neighbor_stats()
    s.close()
    neighbors_ref.check(got, neighbors_ref.reference(oracle, rows, ids, k, part))
    c = pr.model(r.key, r.select).c
    stride, _span_len, spans = pr.neighbor_sample(c.TB, k)
    assert (st["rows"], st["k"], st["tile_rows"], st["sample_stride"], st["spans"]) == (len(rows), k, c.tile, stride, spans)
    assert (stride == 4) == (r.key == "big64") and st["reruns"] == (1 if r.grows else 0)
    held(r, "candidates", st["candidates"], *pr.bracket(r))


def round_log(path):
    """PCV_LINKAGE_ROUNDS_FILE: round, components before and after, candidates, bound repeated at stride 1, list rerun, four times"""
    return [[int(x) for x in line.split()[:6]] for line in open(path).read().splitlines()]


def same_tree(oracle, rows, got_a, got_b, got_c, tree):
    """the returned edges are the model's exact tree, and every c has the oracle's bits"""
    assert {(min(a, b), max(a, b)) for a, b in zip(got_a.tolist(), got_b.tolist())} == \
        {(min(a, b), max(a, b)) for a, b in zip(tree.edges[0].tolist(), tree.edges[1].tolist())}
    want = np.array([oracle.canonical_score(rows[a], rows[b], 0) for a, b in zip(got_a.tolist(), got_b.tolist())])
    np.testing.assert_array_equal(got_c.view(np.uint64), want.view(np.uint64))


def rounds_held(r, log, tree, st, cap):
    """every round of the device's log against the model's: the components before and after it and the repeat of the bound pass for
    equality, the candidates inside the round's bracket, a rerun where they outgrow the list (which keeps the room it grew to);
    -> the reruns"""
    assert st["rounds"] == len(log) == len(tree.rounds)
    reruns = 0
    for (i, before, after, cand, repeated, rerun), m in zip(log, tree.rounds):
        assert (before, after, bool(repeated)) == (m.before, m.after, m.bound_repeated), (i, before, after, repeated, m)
        held(r, "round %d (%d -> %d components)" % (i, before, after), cand, m.lo, m.hi)
        assert rerun == (1 if cand > cap else 0)
        reruns += rerun
        cap = max(cap, cand)
    assert st["candidates"] == sum(x[3] for x in log)
    assert reruns >= 1 or not r.grows
    return reruns


@runs_of("linkage")
def test_linkage(ctx, oracle, tmp_path, monkeypatch, r):
    monkeypatch.setenv("PCV_LINKAGE_ROUNDS_FILE", str(tmp_path / "rounds"))
    s, src, rows, ids, part = open_searcher(ctx, r)
    got = s.linkage_tree(src)
    st = s.last_linkage_stats()
    s.close()
    tree = pr.bracket(r)
    c = pr.model(r.key, r.select).c
    if len(rows) <= MAX_VERIFIED_ROWS:
        linkage_ref.check_verified(oracle, rows, ids, got, part, st)
    same_tree(oracle, rows, got[2], got[3], got[6], tree)
    assert st["tile_rows"] == c.tile and st["participating"] == c.P and (pr.linkage_stride(c.TB) == 4) == (r.key == "big64")
    assert st["reruns"] == rounds_held(r, round_log(tmp_path / "rounds"), tree, st, pr.first_capacity(r, c))
    held(r, "candidates", st["candidates"], *pr.total(tree))


@runs_of("reach")
def test_reach(ctx, oracle, tmp_path, monkeypatch, r):
    monkeypatch.setenv("PCV_LINKAGE_ROUNDS_FILE", str(tmp_path / "rounds"))
    min_items = r.args[0]
    s, src, rows, ids, part = open_searcher(ctx, r)
    got = s.reach_tree(src, min_items)
    st = s.last_reach_stats()
    s.close()
    core, tree = pr.bracket(r)
    c = pr.model(r.key, r.select).c
    reach_ref.check_verified(oracle, rows, ids, got, min_items, part, st)
    assert {(min(a, b), max(a, b)) for a, b in zip(got[3].tolist(), got[4].tolist())} == \
        {(min(a, b), max(a, b)) for a, b in zip(tree.edges[0].tolist(), tree.edges[1].tolist())}
    assert st["tile_rows"] == c.tile and st["participating"] == c.P and st["min_items"] == min_items
    held(r, "core_candidates", st["core_candidates"], *core)
    core_cap = max(65536, 32 * (min_items - 1) * c.rows_selected)  # NeighborPlan::open with k = min_items - 1
    assert not core[0] <= core_cap < core[1]
    core_rerun = 1 if st["core_candidates"] > core_cap else 0
    assert st["reruns"] == core_rerun + rounds_held(r, round_log(tmp_path / "rounds"), tree, st, pr.first_capacity(r, c))
    held(r, "candidates", st["candidates"], *pr.total(tree))


def test_reach_with_min_items_1_lists_what_linkage_lists(ctx, tmp_path, monkeypatch):
    """every core is +inf: the capped screen is the linkage screen, round for round"""
    r = next(x for x in pr.RUNS if x.screen == "linkage" and x.key == "g384")
    s = open_searcher(ctx, r)[0]
    monkeypatch.setenv("PCV_LINKAGE_ROUNDS_FILE", str(tmp_path / "linkage"))
    link = s.linkage_tree(None)
    monkeypatch.setenv("PCV_LINKAGE_ROUNDS_FILE", str(tmp_path / "reach"))
    reach = s.reach_tree(None, 1)
    st = s.last_reach_stats()
    s.close()
    a, b = round_log(tmp_path / "linkage"), round_log(tmp_path / "reach")
    print(a)
    assert a == b and len(a) >= 3
    assert st["core_candidates"] == 0 and st["candidates"] == sum(x[3] for x in a)
    for x, y in zip(link[2:], reach[3:7] + (reach[8],)):
        assert x.tobytes() == y.tobytes()
