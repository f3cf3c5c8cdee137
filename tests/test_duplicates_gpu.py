"""GPU: duplicate pairs (pcv_searcher_find_duplicates), through the Python mirror of the C ABI.  The reference of every check is
orc_canonical_score(row_a, row_b, D, 0) >= (double)threshold over all a < b of the participating rows, sorted (-c, a, b); ids, f32
score bits, count and total are compared for equality.

The reference calls the oracle for every pair whose f64 cosine by numpy is within 1e-6 of the threshold or above it: the two f64
computations differ by D * 2^-53 at most, so a pair further below cannot reach the threshold in the oracle either."""
import os
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from duplicates_ref import bits, build, check, make_ids, neighbour, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D = 384
PCV_ERR_UNSUPPORTED = 3
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


# ---- 1. golden corpora with planted copies and neighbours ------------------------------------------------------------------
def planted_positions(n):
    """(a, b): block and tile edges, the last two rows, one pair inside a 32-row block, one pair 900 rows apart"""
    pairs = [(0, 1), (31, 32), (127, 128), (n - 2, n - 1), (40, 45), (50, 950)]
    return [(a, b) for a, b in pairs if b < n and a >= 0]


# What the golden corpora hold of their own: in scan_n1000_d384 row 777 is row 123 and row 778 is three times row 123 (cosine 1 less
# some 1e-15), and row 500 is a zero row, which pairs with nothing.
NATIVE = {"scan_n77_d100": [], "scan_n1000_d384": [(123, 777), (123, 778), (777, 778)]}


def planted_golden(golden_dir, name, metric, kind):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    rows = np.array(g["corpus"], dtype=np.float32)
    rng = np.random.default_rng(3)
    for a, b in planted_positions(rows.shape[0]):
        rows[b] = rows[a] if kind == "copy" else neighbour(rng, rows[a], 0.999)
    if metric == "dot":
        rows = (rows * rng.uniform(0.5, 1.5, size=(rows.shape[0], 1))).astype(np.float32)
    return np.ascontiguousarray(rows), make_ids(rng, rows.shape[0])


@pytest.mark.parametrize("kind", ["copy", "near"])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("name", ["scan_n77_d100", "scan_n1000_d384"])
def test_golden_planted(ctx, oracle, golden_dir, name, metric, kind):
    rows, ids = planted_golden(golden_dir, name, metric, kind)
    n = rows.shape[0]
    s = build(ctx, rows, ids, metric)
    planted = {(int(ids[a]), int(ids[b])) for a, b in planted_positions(n)}
    native = {(int(ids[a]), int(ids[b])) for a, b in NATIVE[name]}
    # 0.99: the planted pairs and the corpus's own copies alone; the low threshold: hundreds of chance pairs of the Gaussian rows as well
    for thr in (0.99, BELOW_ONE, 0.2 if n == 77 else 0.15):
        got = s.find_duplicates(None, thr)
        want = reference(oracle, rows, ids, thr)
        check(got, want)
        found = set(zip(got[0].tolist(), got[1].tolist()))
        if thr == 0.99:
            assert found == planted | native
        elif thr == BELOW_ONE:
            # (a dot-metric copy is the row times another amplitude, rounded: its cosine falls short of 1 by some 1e-15)
            assert found == (planted if kind == "copy" else set()) | native
        else:
            assert planted | native < found and len(found) > len(planted) + 10
    st = s.last_duplicate_stats()
    assert st["rows"] == n and st["pairs"] == got[3] and st["candidates"] >= st["pairs"] and st["tile_rows"] == 128
    s.close()


# ---- 2. tile and segment edges -----------------------------------------------------------------------------------------------
def test_tile_and_segment_edges(ctx, oracle):
    """Two sources of 33 and 165 rows: partial last blocks, and the tile of blocks 0..3 holds rows of both"""
    rng = np.random.default_rng(8)
    n1, n2 = 33, 165
    rows = rng.standard_normal((n1 + n2, D)).astype(np.float32)
    ids = make_ids(rng, n1 + n2)
    rows[n1 + 100] = rows[20]                             # a cross-source pair
    rows[32] = neighbour(rng, rows[31], 0.999)            # the last row of source 1, alone in its block
    rows[n1] = neighbour(rng, rows[32], 0.9995)           # ... and the first row of source 2: across the boundary (31-33 too)
    rows[n1 + n2 - 1] = rows[n1 + 31]                     # inside source 2, its last row (partial block)
    s = build(ctx, rows, ids, sources=[(1, 0, n1), (2, n1, n1 + n2)])
    assert s.num_segments == 2
    for thr in (0.99, 0.12):
        both = s.find_duplicates(None, thr)
        check(both, reference(oracle, rows, ids, thr))
        check(s.find_duplicates([1, 2], thr), reference(oracle, rows, ids, thr))
        check(s.find_duplicates([2, 1], thr), reference(oracle, rows, ids, thr))
        check(s.find_duplicates([1], thr), reference(oracle, rows, ids, thr, np.arange(n1)))
        check(s.find_duplicates([2], thr), reference(oracle, rows, ids, thr, np.arange(n1, n1 + n2)))
    got = s.find_duplicates(None, 0.99)
    assert got[3] == 5 and (int(ids[20]), int(ids[n1 + 100])) in set(zip(got[0].tolist(), got[1].tolist()))
    assert s.find_duplicates([2], 0.99)[3] == 1 and s.find_duplicates([1], 0.99)[3] == 1  # the cross pairs are gone
    empty = s.find_duplicates([], 0.5)
    assert empty[3] == 0 and len(empty[0]) == 0 and len(empty[1]) == 0 and len(empty[2]) == 0
    assert s.find_duplicates([99], 0.5)[3] == 0
    s.close()


# ---- 3. pairs within 3e-7 of the threshold -----------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.9, BELOW_ONE, 0.5])
@pytest.mark.parametrize("shape", [("cosine", 384), ("dot", 768)])
def test_adversarial_threshold(ctx, oracle, shape, thr):
    metric, dim = shape
    rng = np.random.default_rng(11)
    base = rng.standard_normal((200, dim)).astype(np.float32)
    thr32 = float(np.float32(thr))
    partners = np.empty_like(base)
    for i in range(200):
        partners[i] = neighbour(rng, base[i], min(1.0, thr32 + rng.uniform(-3e-7, 3e-7)))
    rows = np.empty((400, dim), dtype=np.float32)
    rows[0::2], rows[1::2] = base, partners
    if metric == "dot":
        rows = (rows * 10.0 ** rng.uniform(-1.0, 1.0, size=(400, 1))).astype(np.float32)
    rows = np.ascontiguousarray(rows)
    ids = make_ids(rng, 400)
    # the sides, decided by the oracle after construction
    c = np.array([oracle.canonical_score(rows[2 * i], rows[2 * i + 1], 0) for i in range(200)])
    assert (np.abs(c - thr32) < 4e-7).all()
    inside = int((c >= thr32).sum())
    print("threshold %.9g: %d pairs at or above, %d below" % (thr32, inside, 200 - inside))
    assert 10 <= inside <= 190
    s = build(ctx, rows, ids, metric)
    got = s.find_duplicates(None, thr)
    check(got, reference(oracle, rows, ids, thr))
    assert got[3] == inside
    st = s.last_duplicate_stats()
    assert st["candidates"] >= 200 and st["tile_rows"] == (128 if dim == 384 else 64)
    s.close()


# ---- 4. rows that take no part -----------------------------------------------------------------------------------------------
def test_rows_that_take_no_part(ctx, oracle):
    rng = np.random.default_rng(14)
    n = 300
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = make_ids(rng, n)
    rows[5] = 0.0
    rows[6] = 0.0  # two zero rows: no cosine, no pair
    for a, b in ((10, 200), (11, 201), (12, 202), (13, 203)):
        rows[b] = rows[a]
    rows[250] = rows[10]  # a group of three: 10, 200, 250
    s = build(ctx, rows, ids)
    thr = BELOW_ONE

    def fresh(part):
        f = build(ctx, np.ascontiguousarray(rows[part]), ids[part])
        out = f.find_duplicates(None, thr)
        f.close()
        return out

    def same(got, want):
        assert got[3] == want[3]
        for x, y in zip(got[:2], want[:2]):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(bits(got[2]), bits(want[2]))

    everything = np.arange(n)
    full = s.find_duplicates(None, thr)
    check(full, reference(oracle, rows, ids, thr))
    assert full[3] == 6 and int(ids[5]) not in full[0].tolist() + full[1].tolist()
    # hidden: the pairs of row 200 are gone, and come back
    assert s.hide_items([int(ids[200])]) == 1
    part = everything[everything != 200]
    hidden = s.find_duplicates(None, thr)
    check(hidden, reference(oracle, rows, ids, thr, part))
    same(hidden, fresh(part))
    assert hidden[3] == 4
    assert s.unhide_items([int(ids[200])]) == 1
    same(s.find_duplicates(None, thr), full)
    # removed: row 201 is gone for good
    assert s.remove_items([int(ids[201])]) == 1
    part = everything[everything != 201]
    removed = s.find_duplicates(None, thr)
    check(removed, reference(oracle, rows, ids, thr, part))
    same(removed, fresh(part))
    assert removed[3] == 5
    # a view over half the ids (the even positions, 201 among the missing)
    half = part[part % 2 == 0]
    v = s.view(ids[half])
    viewed = v.find_duplicates(None, thr)
    check(viewed, reference(oracle, rows, ids, thr, half))
    same(viewed, fresh(half))
    assert viewed[3] == 4  # (10, 200), (10, 250), (200, 250), (12, 202)
    v.close()
    s.close()


# ---- 5. the same id on two rows --------------------------------------------------------------------------------------------
def test_same_id_on_two_rows(ctx, oracle):
    rng = np.random.default_rng(15)
    rows = rng.standard_normal((70, D)).astype(np.float32)
    ids = make_ids(rng, 70)
    rows[60] = rows[3]
    ids[60] = ids[3]
    s = build(ctx, rows, ids)
    got = s.find_duplicates(None, BELOW_ONE)
    check(got, reference(oracle, rows, ids, BELOW_ONE))
    assert got[3] == 1 and got[0][0] == got[1][0] == ids[3]
    s.close()


# ---- 6. truncation ------------------------------------------------------------------------------------------------------------
def test_truncation_is_a_prefix(ctx, oracle, golden_dir):
    rows, ids = planted_golden(golden_dir, "scan_n1000_d384", "cosine", "near")
    s = build(ctx, rows, ids)
    want = reference(oracle, rows, ids, 0.15)
    total = len(want[0])
    assert total > 100
    check(s.find_duplicates(None, 0.15), want)
    for m in (1, total - 1, total, total + 1):
        check(s.find_duplicates(None, 0.15, max_pairs=m), want, m)
    s.close()


# ---- 7. a list that has to grow --------------------------------------------------------------------------------------------
def test_candidate_list_grows(ctx, oracle):
    """700 identical rows: 244 650 pairs, more than the list of the first launch holds (max(65536, 2 * rows), row_jobs.cpp)"""
    rng = np.random.default_rng(16)
    rows = rng.standard_normal((1000, D)).astype(np.float32)
    where = rng.permutation(1000)[:700]
    rows[where] = rows[where[0]]
    ids = make_ids(rng, 1000)
    s = build(ctx, rows, ids)
    got = s.find_duplicates(None, BELOW_ONE)
    assert got[3] == 700 * 699 // 2 == 244650
    check(got, reference(oracle, rows, ids, BELOW_ONE))
    st = s.last_duplicate_stats()
    print(st)
    assert st["candidates"] >= st["pairs"] == 244650
    if st["candidates"] > max(65536, 2 * 1000):
        assert st["reruns"] >= 1
    # ... and the next call starts small again, with the same result
    again = s.find_duplicates(None, BELOW_ONE, max_pairs=10)
    assert again[3] == 244650 and len(again[0]) == 10
    np.testing.assert_array_equal(again[0], got[0][:10])
    s.close()


# ---- 8. settings change nothing ----------------------------------------------------------------------------------------------
def test_independent_of_settings(ctx, oracle, golden_dir):
    rows, ids = planted_golden(golden_dir, "scan_n1000_d384", "cosine", "near")
    want = reference(oracle, rows, ids, 0.15)
    results = []
    for setting in ("off", "int8", "wave"):
        s = pa.Searcher(ctx, D, "cosine")
        if setting == "wave":
            s.set_kernel("wave")
        else:
            s.set_screening_copy(setting)
        s.add_rows(1, rows, ids)
        s.finalize()
        s.set_candidate_capacity(16)
        s.set_tuning(1)
        results.append(s.find_duplicates(None, 0.15))
        s.close()
    for got in results:
        check(got, want)
        for x, y in zip(got[:3], results[0][:3]):
            assert x.tobytes() == y.tobytes()


# ---- 9. tiles of every size, and a dimension with none ------------------------------------------------------------------------
def test_widest_tile_and_unsupported_dimension(ctx, oracle):
    """Dp = 2496 is the widest row whose 32-row bf16 tile fits the LDS (mfma_pass_queries); Dp = 2560 has no tile"""
    rng = np.random.default_rng(17)
    rows = rng.standard_normal((70, 2496)).astype(np.float32)
    ids = make_ids(rng, 70)
    rows[40] = rows[2]
    rows[69] = neighbour(rng, rows[33], 0.9)
    s = build(ctx, rows, ids)
    for thr in (0.95, 0.8, 0.05):
        check(s.find_duplicates(None, thr), reference(oracle, rows, ids, thr))
    assert s.find_duplicates(None, 0.8)[3] == 2 and s.last_duplicate_stats()["tile_rows"] == 32
    s.close()
    rows = rng.standard_normal((40, 2560)).astype(np.float32)
    s = build(ctx, rows, make_ids(rng, 40))
    before = s.search_vectors(None, 5, rows[:2])
    with pytest.raises(pa.PcvError) as e:
        s.find_duplicates(None, 0.9)
    assert e.value.status == PCV_ERR_UNSUPPORTED and "find_duplicates" in str(e.value)
    after = s.search_vectors(None, 5, rows[:2])  # the searcher stays usable
    for x, y in zip(before, after):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    s.close()


# ---- 10. searches are what they were --------------------------------------------------------------------------------------------
def test_search_results_unchanged_by_a_join(ctx, golden_dir):
    g = np.load(os.path.join(golden_dir, "scan_n1000_d384.npz"))
    rows, ids = planted_golden(golden_dir, "scan_n1000_d384", "cosine", "copy")
    queries = np.array(g["queries"], dtype=np.float32)
    s = build(ctx, rows, ids)
    before = s.search_vectors(None, 10, queries)
    stats_before = s.last_stats()
    assert s.find_duplicates(None, 0.99)[3] == 6 + len(NATIVE["scan_n1000_d384"])
    assert s.last_stats() == stats_before  # the join has counters of its own
    after = s.search_vectors(None, 10, queries)
    for x, y in zip(before, after):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    s.close()


# ---- 11. the C++ mirror -------------------------------------------------------------------------------------------------------
def test_cpp_mirror_duplicates_program():
    src = os.path.join(ROOT, "tests", "cpp", "duplicates_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "duplicates_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "duplicates_mirror_test: ok" in r.stdout
