"""GPU: the paths of the duplicate-pair screen (selfjoin_screen_kernel, find_duplicates) on which test_duplicates_gpu.py has no
pair to lose.  The exact f64 step hides every screen error that adds candidates; the one that shows is a true pair that was never
listed — so each test here puts true pairs on one path: a second span, the edge of the certified margin, every chunk count and tile
size, rows the f32 screen is not certified for, thresholds at the ends of the range, a long segment table.

As in test_duplicates_gpu.py the expected result is duplicates_ref.reference (orc_canonical_score decides every pair) and ids, f32
score bits, count and total are compared for equality.  What makes an input hostile is asserted on the CPU before the GPU is used."""
import itertools

import numpy as np
import pytest

from duplicates_ref import bf16_rne, build, check, make_ids, neighbour, reference, screen_score

pytestmark = pytest.mark.gpu

BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


def f32_at_or_below(c):
    t = np.float32(c)
    return float(t) if float(t) <= c else float(np.nextafter(t, np.float32(-np.inf)))


def f32_above(c):
    t = np.float32(c)
    return float(t) if float(t) > c else float(np.nextafter(t, np.float32(np.inf)))


def pairs_of(got):
    return set(zip(got[0].tolist(), got[1].tolist()))


def id_pairs(ids, groups):
    """every pair inside each group of positions, as (id of the earlier row, id of the later row)"""
    out = set()
    for g in groups:
        for a, b in itertools.combinations(sorted(g), 2):
            out.add((int(ids[a]), int(ids[b])))
    return out


# ---- a. more than one span ------------------------------------------------------------------------------------------------------
def span_corpus():
    """12 320 x 64: 385 blocks.  A work item streams 256 blocks from its tile's first block, so the tiles that start before block
    129 have a second span.  Groups of (block, row of the block): the first is the base, the others copies ('c') or neighbours at
    0.999 ('n') of it, on both sides of the span cut of the base's tile."""
    rng = np.random.default_rng(21)
    n, dim = 12320, 64
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    plan = [
        ((0, 5), [(255, 31, "c"), (256, 0, "n"), (384, 17, "n")]),    # tile of block 0: cut between blocks 255 and 256
        ((4, 7), [(259, 31, "n"), (260, 0, "c")]),                    # tile of block 4: cut between 259 and 260
        ((128, 0), [(383, 12, "c"), (384, 3, "n")]),                  # tile of block 128: its second span is the last block alone
        ((200, 20), [(300, 11, "n")]),                                # a tile with one span
        ((384, 25), [(384, 26, "c")]),                                # inside the last block
    ]
    groups = []
    for (bb, br), partners in plan:
        base = bb * 32 + br
        g = [base]
        for pb, pr, kind in partners:
            at = pb * 32 + pr
            rows[at] = rows[base] if kind == "c" else neighbour(rng, rows[base], 0.999)
            g.append(at)
        groups.append(g)
    return np.ascontiguousarray(rows), make_ids(rng, n), groups


def test_more_than_one_span(ctx, oracle):
    rows, ids, groups = span_corpus()
    n = rows.shape[0]
    assert n == 385 * 32
    planted = id_pairs(ids, groups)
    for g in groups:  # (two neighbours of one row are at 0.998 of each other)
        for a, b in itertools.combinations(g, 2):
            assert oracle.canonical_score(rows[a], rows[b], 0) >= 0.995
    low = 0.55
    want_high, want_low = reference(oracle, rows, ids, 0.99), reference(oracle, rows, ids, low)
    chance = len(want_low[0]) - len(planted)
    print("planted %d, chance pairs at %g: %d" % (len(planted), low, chance))
    assert len(want_high[0]) == len(planted) == 14 and chance >= 20
    s = build(ctx, rows, ids)
    got = s.find_duplicates(None, 0.99)
    check(got, want_high)
    assert pairs_of(got) == planted
    st = s.last_duplicate_stats()
    assert st["reruns"] == 0 and st["rows"] == n and st["tile_rows"] == 128
    got = s.find_duplicates(None, low)
    check(got, want_low)
    assert planted < pairs_of(got)
    assert s.last_duplicate_stats()["reruns"] == 0
    s.close()


# ---- b. rows whose bf16 rounding is all to one side -----------------------------------------------------------------------------
DOWN = 1.0 + 2.0 ** -8 - 2.0 ** -18  # exact in f32; halfway between two bf16 values less 2^-18: rounds down to 1
UP = 1.0 + 2.0 ** -8 + 2.0 ** -18    # rounds up to 1 + 2^-7
N_BIASED = 20                        # pairs of each kind


def biased_pair(rng, dim, mant_a, mant_b, share):
    """a: features +-2^e * mant_a, e in -2..1; b: the same signs with mant_b and the exponents of `share` of the features redrawn"""
    e = rng.integers(-2, 2, size=dim)
    sign = rng.choice([-1.0, 1.0], size=dim)
    m = min(dim, max(1, int(round(dim * share))))
    e2 = e.copy()
    where = rng.permutation(dim)[:m]
    e2[where] = (e[where] + 2 + rng.integers(1, 4, size=m)) % 4 - 2  # another exponent of the four
    a = (sign * np.ldexp(mant_a, e)).astype(np.float32)
    b = (sign * np.ldexp(mant_b, e2)).astype(np.float32)
    assert (a.astype(np.float64) == sign * np.ldexp(mant_a, e)).all() and (b.astype(np.float64) == sign * np.ldexp(mant_b, e2)).all()
    return a, b


def biased_corpus(oracle, dim):
    """400 rows: Gaussian filler and, at random places, N_BIASED 'down' pairs, N_BIASED 'up' pairs and one mixed pair.
    -> rows, ids, {kind: [(a, b, oracle cosine)]} with a < b positions"""
    rng = np.random.default_rng(100 + dim)
    n = 400
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    shares = np.linspace(1.0 / 64, 1.0 / 6, N_BIASED)  # around D/40 features: cosines from about 0.9 to 1
    made = [("down", DOWN, DOWN, sh) for sh in shares] + [("up", UP, UP, sh) for sh in shares] + [("mixed", DOWN, 1.0, 1.0 / 40)]
    places = rng.permutation(n)[: 2 * len(made)]
    out = {"down": [], "up": [], "mixed": []}
    for i, (kind, ma, mb, sh) in enumerate(made):
        pa_, pb_ = sorted((int(places[2 * i]), int(places[2 * i + 1])))
        rows[pa_], rows[pb_] = biased_pair(rng, dim, ma, mb, sh)
        out[kind].append((pa_, pb_))
    rows = np.ascontiguousarray(rows)
    for kind in out:
        out[kind] = [(a, b, oracle.canonical_score(rows[a], rows[b], 0)) for a, b in out[kind]]
    return rows, make_ids(rng, n), out


def check_bias(rows, made):
    """The inputs are as hostile as claimed: the screen's score in exact arithmetic falls short of (down) or exceeds (up) the
    cosine by nearly the whole bf16 part of the certified margin, u (2 + u) = 0.0078278."""
    assert abs((1.0 - DOWN ** -2) - 0.007759) < 1e-6 and abs(((1.0 + 2.0 ** -7) / UP) ** 2 - 1.0 - 0.007790) < 1e-6
    for kind, lo, hi in (("down", 0.00775, 0.0078278), ("up", -0.0078278, -0.00778), ("mixed", 0.0038, 0.0040)):
        ratio = np.array([(c - screen_score(rows[a], rows[b])) / c for a, b, c in made[kind]])
        print("%s: (c - screen) / c in [%.6f, %.6f], cosines %.4f .. %.4f" % (kind, ratio.min(), ratio.max(), min(c for _, _, c in made[kind]), max(c for _, _, c in made[kind])))
        assert (ratio >= lo).all() and (ratio <= hi).all()
    for kind in ("down", "up"):
        c = np.array([c for _, _, c in made[kind]])
        assert c.min() < 0.95 and c.max() > 0.985 and c.max() < 1.0 and c.min() > 0.85
        assert len({(a // 32, b // 32) for a, b, _ in made[kind]}) >= N_BIASED - 4  # spread over the blocks
    a, b, _ = made["mixed"][0]
    assert (bf16_rne(rows[b]) == rows[b]).all() and (bf16_rne(rows[a]) != rows[a]).all()


@pytest.mark.parametrize("dim", [64, 384, 768, 2496])
def test_rounding_biased_rows_stay_inside_the_margin(ctx, oracle, dim):
    rows, ids, made = biased_corpus(oracle, dim)
    check_bias(rows, made)
    s = build(ctx, rows, ids)

    def three(kind):
        by_c = sorted(made[kind], key=lambda p: p[2])
        return [by_c[0], by_c[len(by_c) // 2], by_c[-1]]

    # a down pair AT the threshold: the screen sees it 0.00776 c below and must still list it
    for a, b, c in three("down") + made["mixed"]:
        thr = f32_at_or_below(c)
        got = s.find_duplicates(None, thr)
        check(got, reference(oracle, rows, ids, thr))
        assert (int(ids[a]), int(ids[b])) in pairs_of(got)
    # an up pair just BELOW the threshold: the screen sees it 0.00779 c above, lists it, and the f64 step drops it
    for a, b, c in three("up"):
        thr = f32_above(c)
        assert c < thr <= 1.0
        got = s.find_duplicates(None, thr)
        check(got, reference(oracle, rows, ids, thr))
        assert (int(ids[a]), int(ids[b])) not in pairs_of(got)
        st = s.last_duplicate_stats()
        assert st["candidates"] > st["pairs"]
    assert s.last_duplicate_stats()["tile_rows"] == {64: 128, 384: 128, 768: 64, 2496: 32}[dim]
    s.close()


# ---- c. every chunk count and both sides of the tile-size boundaries ----------------------------------------------------------------
TILE_ROWS = {50: 128, 130: 128, 576: 128, 640: 64, 1216: 64, 1280: 32}  # Dp 64 (one chunk), 192, 576 | 640, 1216 | 1280


def chunk_corpus(dim):
    """800 rows, 25 blocks with the last one partial: a wave streams three or four blocks.  Copies of row 3 in its block, in the next
    block, in the first block of the next tile, 8, 9, 16 and 17 blocks on (a wave's second and third block and their neighbours) and
    in the last block."""
    rng = np.random.default_rng(300 + dim)
    n = 800
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    nt = TILE_ROWS[dim] // 32
    blocks = sorted({1, nt, 8, 9, 16, 17, 24})
    group = [3, 20] + [b * 32 + (5 * b + 1) % 32 for b in blocks]
    assert group[-1] < n and len(set(group)) == len(group)
    for at in group[1:]:
        rows[at] = rows[3]
    return np.ascontiguousarray(rows), make_ids(rng, n), group


@pytest.mark.parametrize("dim", sorted(TILE_ROWS))
def test_every_chunk_count_and_tile_boundary(ctx, oracle, dim):
    rows, ids, group = chunk_corpus(dim)
    planted = id_pairs(ids, [group])
    low = 3.0 / np.sqrt(dim)
    want_high, want_low = reference(oracle, rows, ids, 0.99), reference(oracle, rows, ids, low)
    chance = len(want_low[0]) - len(planted)
    print("%d-d: planted %d, chance pairs at %.4f: %d" % (dim, len(planted), low, chance))
    # 319 600 pairs at three standard deviations of the cosine of two Gaussian rows: 431 expected in the normal limit
    assert len(want_high[0]) == len(planted) and chance >= 200
    s = build(ctx, rows, ids)
    got = s.find_duplicates(None, 0.99)
    check(got, want_high)
    assert pairs_of(got) == planted
    assert s.last_duplicate_stats()["tile_rows"] == TILE_ROWS[dim]
    got = s.find_duplicates(None, low)
    check(got, want_low)
    assert planted < pairs_of(got)
    s.close()


# ---- d. rows the f32 screen is not certified for, and rows at the edge of having a cosine -------------------------------------------
WILD_DIM = 384
SITES = (-63, -20, 20, 60)  # |x| of a scaled copy, as a power of two times (1 +- 2^-12)


def canonical_norm2(x):
    return float(np.cumsum(x.astype(np.float64) ** 2)[-1])


def wild_corpus(oracle):
    """200 rows.  Eight base rows with |x| = 2^m (1 + 2^-12) ('hi', four of them) or 2^m (1 - 2^-12) ('lo'), a 0.999-neighbour of
    each, and copies of each base times exact powers of two that put |x| beside 2^-63 (|x|^2 beside 2^-126, the edge of having a
    cosine), beside 2^-20 and 2^20 (the edges of the certified f32 screen) and beside 2^60.
    -> rows, ids, groups [(base, neighbour, {site: position})], defined (bool per row), wild (bool per row)"""
    rng = np.random.default_rng(41)
    n = 200
    rows = rng.standard_normal((n, WILD_DIM)).astype(np.float32)
    places = rng.permutation(n)[: 8 * 6].reshape(8, 6)
    defined = np.ones(n, dtype=bool)
    wild = np.zeros(n, dtype=bool)
    groups = []
    for i in range(8):
        hi = i < 4
        base, nb = int(places[i, 0]), int(places[i, 1])
        x = rows[base].astype(np.float64)
        m = int(np.ceil(np.log2(np.linalg.norm(x))))
        x = (x * (2.0 ** m * (1.0 + (2.0 ** -12 if hi else -(2.0 ** -12))) / np.linalg.norm(x))).astype(np.float32)
        norm = np.sqrt(canonical_norm2(x))
        assert (2.0 ** m < norm < 2.0 ** m * (1 + 2.0 ** -11)) if hi else (2.0 ** m * (1 - 2.0 ** -11) < norm < 2.0 ** m)
        rows[base] = x
        rows[nb] = neighbour(rng, x, 0.999)
        copies = {}
        for j, site in enumerate(SITES):
            at = int(places[i, 2 + j])
            y = np.ldexp(x, site - m)
            # every feature a normal f32: the scaling is exact
            assert y.dtype == np.float32 and (np.abs(y) >= 2.0 ** -126).all() and np.isfinite(y).all()
            assert (y.astype(np.float64) == x.astype(np.float64) * 2.0 ** (site - m)).all()
            rows[at] = y
            copies[site] = at
            n2 = canonical_norm2(y)
            # where the scaled norm lands (selfjoin_prep_kernel: a cosine iff |x|^2 >= 2^-126, certified iff 2^-40 <= |x|^2 <= 2^40)
            assert n2 == canonical_norm2(x) * 4.0 ** (site - m)
            assert (n2 > 4.0 ** site) if hi else (n2 < 4.0 ** site)
            assert abs(n2 / 4.0 ** site - 1.0) < 2.0 ** -10
            defined[at] = n2 >= 2.0 ** -126
            wild[at] = defined[at] and not (2.0 ** -40 <= n2 <= 2.0 ** 40)
            assert bool(defined[at]) == (hi or site != -63)
            assert bool(wild[at]) == (defined[at] and (site in (-63, 60) or (site == 20 and hi) or (site == -20 and not hi)))
        groups.append((base, nb, copies))
    rows = np.ascontiguousarray(rows)
    for base, nb, copies in groups:
        for site, at in copies.items():
            if defined[at]:
                # the oracle's cosine of a scaled pair has the bits of the unscaled pair's
                assert oracle.canonical_score(rows[at], rows[nb], 0) == oracle.canonical_score(rows[base], rows[nb], 0)
                assert oracle.canonical_score(rows[base], rows[at], 0) == oracle.canonical_score(rows[base], rows[base], 0)
            else:
                assert np.isnan(oracle.canonical_score(rows[at], rows[nb], 0))
    return rows, make_ids(rng, n), groups, defined, wild


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_wild_and_barely_defined_rows(ctx, oracle, metric):
    rows, ids, groups, defined, wild = wild_corpus(oracle)
    n_part, n_wild = int(defined.sum()), int(wild.sum())
    assert n_part == 196 and n_wild == 20
    s = build(ctx, rows, ids, metric)
    for thr, with_neighbour in ((BELOW_ONE, False), (0.99, True)):
        expected = id_pairs(ids, [[base] + ([nb] if with_neighbour else []) + [at for at in copies.values() if defined[at]]
                                  for base, nb, copies in groups])
        got = s.find_duplicates(None, thr)
        check(got, reference(oracle, rows, ids, thr))
        assert pairs_of(got) == expected and len(expected) == (100 if with_neighbour else 64)
        st = s.last_duplicate_stats()
        print(st)
        # every pair of a wild row with a participating row is a candidate (the pairs of two wild rows counted once)
        assert st["candidates"] >= n_wild * (n_part - n_wild) + n_wild * (n_wild - 1) // 2
        undefined = {int(ids[i]) for i in np.nonzero(~defined)[0]}
        assert not undefined & (set(got[0].tolist()) | set(got[1].tolist()))
    s.close()


# ---- e. thresholds at the ends of the range ---------------------------------------------------------------------------------------------
def test_threshold_edges(ctx, oracle):
    rng = np.random.default_rng(51)
    rows = rng.standard_normal((60, 100)).astype(np.float32)
    ids = make_ids(rng, 60)
    rows[47] = rows[9]
    rows[58] = rows[33]
    s = build(ctx, rows, ids)
    # 1.0: what the oracle says of the copies; 0.005: the screen threshold is negative; -0.999: all but the most opposed pairs
    for thr in (1.0, 0.0, 0.005, -0.5, -0.999):
        want = reference(oracle, rows, ids, thr)
        got = s.find_duplicates(None, thr)
        check(got, want)
        st = s.last_duplicate_stats()
        assert st["candidates"] >= st["pairs"] == len(want[0])
    assert len(want[0]) > 60 * 59 // 2 - 10
    s.close()


# ---- f. a long segment table ------------------------------------------------------------------------------------------------------------
def test_long_segment_table(ctx, oracle):
    """Seven sources of 1, 31, 32, 33, 64, 300 and 5 rows: find_seg's binary search and join_seek's forward walk over a table of
    seven entries, segments shorter than a block in the middle of it, a source emptied by remove_items, and a view."""
    rng = np.random.default_rng(61)
    sizes = [1, 31, 32, 33, 64, 300, 5]
    first = np.concatenate([[0], np.cumsum(sizes)])
    n = int(first[-1])
    dim = 384
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    ids = make_ids(rng, n)

    def at(source, r):  # position of row r of source 1..7
        assert 0 <= r < sizes[source - 1]
        return int(first[source - 1]) + r

    copies = [
        (at(1, 0), at(2, 30)), (at(2, 4), at(3, 0)), (at(3, 31), at(4, 32)), (at(4, 7), at(5, 63)), (at(5, 20), at(6, 299)),
        (at(6, 150), at(7, 4)),                    # across every neighbouring pair of sources
        (at(1, 0), at(7, 0)),                      # the first source and the last (with the first line: a group of three)
        (at(6, 10), at(6, 200)), (at(6, 31), at(6, 32)),  # inside the 300-row source
    ]
    for a, b in copies:
        rows[b] = rows[a]
    rows = np.ascontiguousarray(rows)
    sources = [(i + 1, int(first[i]), int(first[i + 1])) for i in range(7)]
    s = build(ctx, rows, ids, sources=sources)
    assert s.num_segments == 7

    def rows_of(listed, gone=()):
        return np.concatenate([np.arange(first[i - 1], first[i]) for i in sorted(set(listed)) if i not in gone] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)

    def run(searcher, listed, part):
        for thr in (0.99, 0.12):
            got = searcher.find_duplicates(listed, thr)
            check(got, reference(oracle, rows, ids, thr, part))
        return got

    everything = list(range(1, 8))
    assert len(reference(oracle, rows, ids, 0.99)[0]) == len(copies) + 1 and len(reference(oracle, rows, ids, 0.12)[0]) > 300
    run(s, None, None)
    run(s, [7, 1, 4], rows_of([7, 1, 4]))
    run(s, [6], rows_of([6]))
    run(s, everything[::-1], None)
    assert s.find_duplicates([7, 1, 4], 0.99)[3] == 1 and s.find_duplicates([6], 0.99)[3] == 2
    # the 32-row source emptied: its entry leaves the table and the blocks behind it move up
    assert s.remove_items(ids[first[2]:first[3]]) == 32
    run(s, None, rows_of(everything, gone=(3,)))
    run(s, [3, 2, 4], rows_of([2, 4]))
    assert s.find_duplicates([3], 0.5)[3] == 0
    assert s.find_duplicates(None, 0.99)[3] == len(copies) + 1 - 2
    # a view over the ids of three sources
    part = rows_of([2, 5, 6])
    v = s.view(ids[part])
    run(v, None, part)
    assert v.find_duplicates(None, 0.99)[3] == 3
    v.close()
    s.close()
