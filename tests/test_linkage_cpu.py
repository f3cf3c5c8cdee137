"""CPU: the linkage tree (pcv_searcher_linkage_tree, pcv_searcher_last_linkage_stats, pcv_linkage_cut) is declared, exported, bound
and present in the regenerated Rust ffi; the argument checks need no GPU; pcv_linkage_cut, which needs none at all, agrees with the
cut written in plain Python and with the density clusters' reference; and the reference and the verifier the GPU tests compare with
(linkage_ref.py) give the answers written out here by hand — the verifier also refuses three wrong trees."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import density_ref
import perceive_amd as pa
from linkage_ref import cut, reference, verify
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
ARITY = {"pcv_searcher_linkage_tree": 13, "pcv_searcher_last_linkage_stats": 2, "pcv_linkage_cut": 10}
STATS = ["rows", "participating", "edges", "candidates", "rounds", "tile_rows", "reruns", "prep_ms", "bound_ms", "list_ms", "rescore_ms", "merge_ms"]


def test_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "perceive_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pcv_[a-z0-9_]+)", out))
    lib = _ffi.lib()
    for name, arity in ARITY.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == arity
        assert name in exported
        assert name in _ffi.SYMBOLS and getattr(lib, name).argtypes
        assert len(_ffi.SYMBOLS[name][1]) == arity
    m = re.search(r"\bpcv_searcher_linkage_tree\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "pcv_searcher* s", "const int64_t* source_ids", "int n_sources", "int64_t capacity", "int64_t* out_ids", "int8_t* out_part",
        "int64_t* out_pos_a", "int64_t* out_pos_b", "int64_t* out_id_a", "int64_t* out_id_b", "double* out_c", "int64_t* out_rows",
        "int64_t* out_edges"]
    m = re.search(r"\bpcv_linkage_cut\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "const int64_t* pos_a", "const int64_t* pos_b", "const double* c", "int64_t n_edges", "const int8_t* part", "int64_t n_rows",
        "double threshold", "int64_t min_clusters", "int32_t* out_label", "int32_t* out_clusters"]
    # the stats struct: the header's fields, in order, with the binding's widths
    m = re.search(r"typedef struct pcv_linkage_stats \{(.*?)\} pcv_linkage_stats;", header, flags=re.S)
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, widths[t]) for n, t in fields] == list(_ffi.LinkageStats._fields_)
    assert [n for n, _ in fields] == STATS
    assert [t for _, t in fields] == ["int64_t"] * 4 + ["int32_t"] * 3 + ["float"] * 5
    assert C.sizeof(_ffi.LinkageStats) == 64


def test_regenerated_rust_ffi_is_current():
    ffi_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")).read()
    assert ("pub fn pcv_searcher_linkage_tree(s: *mut pcv_searcher, source_ids: *const i64, n_sources: c_int, capacity: i64, out_ids: *mut i64, "
            "out_part: *mut int8_t, out_pos_a: *mut i64, out_pos_b: *mut i64, out_id_a: *mut i64, out_id_b: *mut i64, out_c: *mut f64, "
            "out_rows: *mut i64, out_edges: *mut i64) -> c_int;") in ffi_rs
    assert "pub fn pcv_searcher_last_linkage_stats(s: *mut pcv_searcher, out: *mut pcv_linkage_stats) -> c_int;" in ffi_rs
    assert ("pub fn pcv_linkage_cut(pos_a: *const i64, pos_b: *const i64, c: *const f64, n_edges: i64, part: *const int8_t, n_rows: i64, "
            "threshold: f64, min_clusters: i64, out_label: *mut i32, out_clusters: *mut i32) -> c_int;") in ffi_rs
    want = r"pub struct pcv_linkage_stats \{\s*" + r"\s*".join(
        r"pub %s: %s," % (n, "i64" if i < 4 else "i32" if i < 7 else "f32") for i, n in enumerate(STATS)) + r"\s*\}"
    assert re.search(want, ffi_rs)
    # ... and the file is what the generator writes from the header today
    import importlib.util
    import tempfile

    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with tempfile.TemporaryDirectory() as tmp:
        gen.OUT = os.path.join(tmp, "ffi.rs")
        gen.main()
        assert open(gen.OUT).read() == ffi_rs


def test_bad_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    fake = C.c_void_p(1)  # never dereferenced: the argument checks come first
    i64 = {k: np.full(4, -77, dtype=np.int64) for k in ("ids", "pos_a", "pos_b", "id_a", "id_b")}
    part = np.full(4, -77, dtype=np.int8)
    c = np.full(4, -77.0, dtype=np.float64)
    rows, edges = C.c_int64(-5), C.c_int64(-5)
    arrays = dict({k + "_p": _ffi.i64p(v) for k, v in i64.items()}, part_p=_ffi.i8p(part), c_p=_ffi.f64p(c), edges_p=C.byref(edges))
    nothing = {k: None for k in arrays}

    def call(s, capacity=4, rows_p=C.byref(rows), **kw):
        a = dict(arrays, **kw)
        return lib.pcv_searcher_linkage_tree(s, None, 0, capacity, a["ids_p"], a["part_p"], a["pos_a_p"], a["pos_b_p"], a["id_a_p"], a["id_b_p"],
                                             a["c_p"], rows_p, a["edges_p"])

    def message():
        msg = lib.pcv_last_error().decode()
        assert "linkage_tree" in msg
        return msg

    assert call(None) == PCV_ERR_INVALID
    assert "searcher is NULL" in message()
    assert call(None, capacity=0, **nothing) == PCV_ERR_INVALID  # counting only, too
    assert "searcher is NULL" in message()
    assert call(fake, rows_p=None) == PCV_ERR_INVALID
    assert "out_rows is NULL" in message()
    for cap in (-1, -(1 << 40)):
        assert call(fake, capacity=cap) == PCV_ERR_INVALID
        assert "capacity %d is negative" % cap in message()
    for name in ("pos_a_p", "pos_b_p", "c_p", "edges_p"):  # (out_ids, out_part and the edges' ids may be NULL)
        assert call(fake, **{name: None}) == PCV_ERR_INVALID
        assert "is NULL with capacity 4" in message()
    for name in ("id_a_p", "id_b_p"):  # ... the edges' ids both or neither
        assert call(fake, **{name: None}) == PCV_ERR_INVALID
        assert "one of out_id_a and out_id_b" in message()
    assert call(fake, capacity=4, **nothing) == PCV_ERR_INVALID  # counting only means capacity 0
    for name in ("ids_p", "part_p", "id_a_p", "c_p"):  # ... and every array NULL
        assert call(fake, capacity=0, **dict(nothing, **{name: arrays[name]})) == PCV_ERR_INVALID
    assert rows.value == -5 and edges.value == -5  # nothing was written
    assert all((v == -77).all() for v in i64.values()) and (part == -77).all() and (c == -77.0).all()
    st = _ffi.LinkageStats()
    assert lib.pcv_searcher_last_linkage_stats(None, C.byref(st)) == PCV_ERR_INVALID
    assert lib.pcv_searcher_last_linkage_stats(fake, None) == PCV_ERR_INVALID
    assert b"last_linkage_stats" in lib.pcv_last_error()


def test_python_cpp_and_rust_surfaces():
    for cls in (pa.Searcher, pa.SearcherView):
        for name in ("linkage_tree", "last_linkage_stats"):
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("linkage_tree", "last_linkage_stats"):
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited
    assert callable(pa.linkage_cut)
    src = open(os.path.join(ROOT, "perceive_amd", "search.py")).read()
    body = src[src.index("    def linkage_tree("):src.index("    def last_linkage_stats(")]
    assert body.count("pcv_searcher_linkage_tree(") == 2  # the count, then the tree
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn linkage_tree\(&self,\s*sources: &\[i64\]\) -> \(Vec<\(i64, bool\)>, Vec<\(i64, i64, f64\)>\)(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::linkage_tree"
    assert m.group(1).count("ffi::pcv_searcher_linkage_tree(") == 2
    assert search_rs.index("pub fn linkage_tree(") < search_rs.index("impl Drop for Searcher")
    assert re.search(r"\npub fn linkage_cut\(", search_rs) and search_rs.count("ffi::pcv_linkage_cut(") == 1
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count(" linkage_tree(") == 2 and hpp.count("pcv_searcher_linkage_tree(") == 2  # Searcher and SearcherView; the count, then the tree
    assert hpp.count(" last_linkage_stats(") == 2 and hpp.count("inline LinkageCut linkage_cut(") == 1


def test_cpp_mirror_linkage_program_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "linkage_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "linkage_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


# ---- the reference against trees written out by hand ------------------------------------------------------------------------------
def plane_rows(degrees, dim=8, seed=3):
    """rows in one plane of a dim-d space at the given angles, of several lengths: the cosine of two is cos(angle difference)"""
    rng = np.random.default_rng(seed)
    t = np.deg2rad(np.asarray(degrees, dtype=np.float64))
    rows = np.zeros((len(degrees), dim))
    rows[:, 2] = np.cos(t)
    rows[:, 5] = np.sin(t)
    return np.ascontiguousarray((rows * rng.uniform(0.5, 2.0, size=(len(degrees), 1))).astype(np.float32))


ANGLES = [40, 0, 3, 10, 44, 21, 90, 47]  # sorted: 0 3 10 21 40 44 47 90 — gaps 3 7 11 19 4 3 43: no two equal but the two 3s,
#                                           which the f32 rounding of the rows tells apart or the positions do


def test_reference_on_points_of_a_plane(oracle):
    """On a line of angles the tree is the path through the sorted angles, and its edges come out by ascending gap."""
    rows = plane_rows(ANGLES)
    ids = np.arange(8, dtype=np.int64) * 11 + 5
    got = reference(oracle, rows, ids)
    assert got[0].tolist() == ids.tolist() and got[1].tolist() == [1] * 8
    edges = list(zip(got[2].tolist(), got[3].tolist()))
    # gaps: 3 (1-2), 3 (4-7: 44-47), 4 (0-4: 40-44), 7 (2-3), 11 (3-5), 19 (0-5: 21-40), 43 (6-7: 47-90)
    assert sorted(edges[:2]) == [(1, 2), (4, 7)]
    assert edges[2:] == [(0, 4), (2, 3), (3, 5), (0, 5), (6, 7)]
    assert got[4].tolist() == ids[got[2]].tolist() and got[5].tolist() == ids[got[3]].tolist()
    assert (np.diff(got[6]) <= 0).all()
    assert np.abs(got[6] - np.cos(np.deg2rad([3, 3, 4, 7, 11, 19, 43]))).max() < 1e-6
    for a, b, c in zip(*got[2:4], got[6]):
        assert c == oracle.canonical_score(rows[a], rows[b], 0)
    assert verify(oracle, rows, got[1], (got[2], got[3], got[6])) is None
    # rows that take no part: a zero row, a row with a NaN, a hidden row.  The path closes over them
    rows2 = rows.copy()
    rows2[3] = 0.0
    rows2[4, 1] = np.nan
    part = np.ones(8, dtype=bool)
    part[7] = False
    got = reference(oracle, rows2, ids, part)
    assert got[1].tolist() == [1, 1, 1, 0, 0, 1, 1, 0]
    # left: 40, 0, 3, 21, 90 -> gaps 3 (1-2), 18 (2-5), 19 (0-5), 50 (0-6)
    assert list(zip(got[2].tolist(), got[3].tolist())) == [(1, 2), (2, 5), (0, 5), (0, 6)]
    assert verify(oracle, rows2, got[1], (got[2], got[3], got[6])) is None
    # one participating row, and none
    got = reference(oracle, rows[:1], ids[:1])
    assert got[1].tolist() == [1] and len(got[2]) == len(got[6]) == 0
    got = reference(oracle, np.zeros((3, 8), dtype=np.float32), ids[:3])
    assert got[1].tolist() == [0, 0, 0] and len(got[6]) == 0
    got = reference(oracle, np.zeros((0, 8), dtype=np.float32), ids[:0])
    assert len(got[0]) == len(got[1]) == len(got[6]) == 0


def star_rows():
    return np.ascontiguousarray(np.eye(64, dtype=np.float32)[:, ::-1] * np.float32(3.0))  # 64 orthonormal directions, every c exactly 0


def test_reference_on_the_star(oracle):
    """Every c is exactly 0: the order is the positions' alone, and Kruskal takes (0,1), (0,2), ..., (0,63)."""
    rows = star_rows()
    got = reference(oracle, rows, np.arange(64, dtype=np.int64))
    assert got[2].tolist() == [0] * 63 and got[3].tolist() == list(range(1, 64))
    assert (got[6] == 0.0).all() and not np.signbit(got[6]).any()
    assert verify(oracle, rows, got[1], (got[2], got[3], got[6])) is None


def test_verify_rejects_wrong_trees(oracle):
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((90, 16)).astype(np.float32)
    rows[40] = rows[7] * np.float32(2.0)  # c(7, 40) = c(7, 7): ties with nothing else, but a clear best edge
    ids = np.arange(90, dtype=np.int64)
    _ids, part, pa_, pb_, _ia, _ib, c = reference(oracle, rows, ids)
    assert verify(oracle, rows, part, (pa_, pb_, c)) is None
    assert (pa_[0], pb_[0]) == (7, 40)

    def score(a, b):
        return oracle.canonical_score(rows[a], rows[b], 0)

    def sorted_edges(edges):
        edges = sorted(edges, key=lambda e: (-e[2], e[0], e[1]))
        return (np.array([e[0] for e in edges], dtype=np.int64), np.array([e[1] for e in edges], dtype=np.int64),
                np.array([e[2] for e in edges], dtype=np.float64))

    edges = list(zip(pa_.tolist(), pb_.tolist(), c.tolist()))
    # 1. one edge swapped for a worse one that spans the same cut: drop the last edge (it joins two components X, Y) and take the
    #    worst pair of X x Y instead — still a spanning tree, every c still the oracle's
    a, b, _c = edges[-1]
    parent = list(range(90))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for x, y, _ in edges[:-1]:
        parent[find(y)] = find(x)
    X = [r for r in range(90) if find(r) == find(a)]
    Y = [r for r in range(90) if find(r) == find(b)]
    assert len(X) + len(Y) == 90 and len(X) * len(Y) > 1
    worse = min(((score(min(x, y), max(x, y)), min(x, y), max(x, y)) for x in X for y in Y))
    assert worse[0] < edges[-1][2]
    verdict = verify(oracle, rows, part, sorted_edges(edges[:-1] + [(worse[1], worse[2], worse[0])]))
    assert verdict is not None and "better pair" in verdict
    # 2. a non-spanning edge set: the last edge swapped for a pair inside X (or Y) — 89 edges that leave two components
    Z = X if len(X) > 2 else Y
    in_tree = {(e[0], e[1]) for e in edges}
    inner = next((x, y) for x in Z for y in Z if x < y and (x, y) not in in_tree)
    verdict = verify(oracle, rows, part, sorted_edges(edges[:-1] + [(inner[0], inner[1], score(*inner))]))
    assert verdict is not None and ("cycle" in verdict or "better pair" in verdict)
    verdict = verify(oracle, rows, part, sorted_edges(edges[:-1] + [edges[0]]))  # ... and for an edge listed twice
    assert verdict is not None
    # 3. too few edges, and a c that is not the oracle's
    assert "edges for" in verify(oracle, rows, part, (pa_[:-1], pb_[:-1], c[:-1]))
    c2 = c.copy()
    c2[5] = np.nextafter(c2[5], 2.0)
    assert "the oracle says" in verify(oracle, rows, part, (pa_, pb_, c2))


def test_verify_rejects_a_tie_broken_the_wrong_way(oracle):
    """The star: every pair has c = 0, so only the positions order the edges.  The path 0-1-2-...-63 is a spanning tree of the same
    total weight, and wrong; so is the star with one edge (0, 63) traded for (1, 63)."""
    rows = star_rows()
    part = np.ones(64, dtype=np.int8)
    zeros = np.zeros(63)
    path = (np.arange(63, dtype=np.int64), np.arange(1, 64, dtype=np.int64), zeros)
    verdict = verify(oracle, rows, part, path)
    assert verdict is not None and "better pair" in verdict
    a = np.zeros(63, dtype=np.int64)
    b = np.arange(1, 64, dtype=np.int64)
    a[62] = 1  # (1, 63) in place of (0, 63): sorted (0,1) ... (0,62), (1,63)
    verdict = verify(oracle, rows, part, (a, b, zeros))
    assert verdict is not None and "(0, 63" in verdict
    # the edges of the right tree in another order are refused as well
    a = np.zeros(63, dtype=np.int64)
    b = np.arange(1, 64, dtype=np.int64)[::-1].copy()
    assert "edge order" in verify(oracle, rows, part, (a, b, zeros))


# ---- pcv_linkage_cut against cut() -------------------------------------------------------------------------------------------------
def random_tree(rng, n, part):
    """a random spanning tree of the rows with part != 0, with descending weights, some of them equal"""
    live = np.nonzero(part)[0]
    order = rng.permutation(live)
    edges = []
    for i in range(1, len(order)):
        j = int(rng.integers(0, i))
        a, b = sorted((int(order[i]), int(order[j])))
        edges.append((a, b))
    c = np.sort(np.round(rng.uniform(-0.5, 1.0, size=len(edges)), 2))[::-1].copy()
    return (np.array([e[0] for e in edges], dtype=np.int64).reshape(-1), np.array([e[1] for e in edges], dtype=np.int64).reshape(-1), c)


def test_linkage_cut_against_the_plain_python_cut():
    rng = np.random.default_rng(5)
    for n, holes in ((1, 0), (2, 0), (9, 0), (40, 0), (40, 7), (200, 31)):
        part = np.ones(n, dtype=np.int8)
        part[rng.permutation(n)[:holes]] = 0
        edges = random_tree(rng, n, part)
        E = len(edges[2])
        assert E == int(part.sum()) - 1
        thresholds = [-np.inf, np.inf, -0.7, 1.5] + sorted(set(edges[2].tolist()))[:: max(1, E // 6)]
        thresholds += [float(np.nextafter(t, 2.0)) for t in thresholds[4:6]]  # just above an edge's c: the edge goes
        for thr in thresholds:
            for K in (1, 2, 5, E, E + 1, E + 7):
                if K < 1:
                    continue
                want = cut(n, part, edges, thr, K)
                got = pa.linkage_cut(*edges, n, part if holes else None, thr, K)
                assert got[0].dtype == np.int32 and got[0].tolist() == want[0].tolist() and got[1] == want[1], (n, holes, thr, K)
        # the K form: exactly K clusters for K up to the participating rows; a threshold equal to an edge's c keeps the edge
        P = int(part.sum())
        for K in range(1, P + 1):
            labels, clusters = pa.linkage_cut(*edges, n, part, -np.inf, K)
            assert clusters == K and len(set(labels[part != 0].tolist())) == K and (labels[part == 0] == -1).all()
        if E:
            t = float(edges[2][E // 2])
            kept = int((edges[2] >= t).sum())
            assert pa.linkage_cut(*edges, n, part, t, 1)[1] == P - kept
            assert pa.linkage_cut(*edges, n, part, float(np.nextafter(t, 2.0)), 1)[1] == P - int((edges[2] > t).sum())


def test_linkage_cut_numbers_clusters_by_their_lowest_position():
    # positions 0..6, 2 takes no part.  Edges best first: 3-5 (0.9), 1-6 (0.8), 0-5 (0.5), 1-3 (0.1), 4-6 (-0.2)
    part = np.array([1, 1, 0, 1, 1, 1, 1], dtype=np.int8)
    edges = (np.array([3, 1, 0, 1, 4]), np.array([5, 6, 5, 3, 6]), np.array([0.9, 0.8, 0.5, 0.1, -0.2]))
    assert pa.linkage_cut(*edges, 7, part, 0.6)[0].tolist() == [0, 1, -1, 2, 3, 2, 1]
    assert pa.linkage_cut(*edges, 7, part, 0.5)[0].tolist() == [0, 1, -1, 0, 2, 0, 1]
    assert pa.linkage_cut(*edges, 7, part, -np.inf, 2)[0].tolist() == [0, 0, -1, 0, 1, 0, 0]
    assert pa.linkage_cut(*edges, 7, part, 0.85, 3)[0].tolist() == [0, 1, -1, 2, 3, 2, 4]  # both rules at once: the stricter one holds
    assert pa.linkage_cut(*edges, 7, part)[1] == 1
    # P = 0 and P = 1, and no rows at all
    none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
    assert pa.linkage_cut(*none, 3, np.zeros(3, dtype=np.int8), 0.5)[0].tolist() == [-1, -1, -1]
    assert pa.linkage_cut(*none, 3, np.zeros(3, dtype=np.int8), 0.5)[1] == 0
    labels, clusters = pa.linkage_cut(*none, 3, np.array([0, 1, 0], dtype=np.int8), 0.5)
    assert labels.tolist() == [-1, 0, -1] and clusters == 1
    labels, clusters = pa.linkage_cut(*none, 0)
    assert len(labels) == 0 and clusters == 0
    assert pa.linkage_cut(*none, 4)[0].tolist() == [0, 1, 2, 3]  # part None: every row takes part


def test_linkage_cut_refuses_bad_input():
    part = np.array([1, 1, 0, 1, 1, 1, 1], dtype=np.int8)
    good = (np.array([3, 1, 0, 1, 4]), np.array([5, 6, 5, 3, 6]), np.array([0.9, 0.8, 0.5, 0.1, -0.2]))

    def refused(a, b, c, n=7, part=part, thr=0.5, K=1):
        with pytest.raises(pa.PcvError) as e:
            pa.linkage_cut(a, b, c, n, part, thr, K)
        assert e.value.status == PCV_ERR_INVALID and "linkage_cut" in str(e.value)
        return str(e.value)

    a, b, c = good
    assert "not ordered" in refused(a, b, np.array([0.9, 0.8, 0.5, 0.6, -0.2]))          # c rises
    assert "not ordered" in refused(a, b, np.array([0.9, 0.8, np.nan, 0.1, -0.2]))       # a NaN
    assert "positions" in refused(np.array([3, 1, 5, 1, 4]), np.array([5, 6, 0, 3, 6]), c)  # pos_a > pos_b
    assert "positions" in refused(np.array([3, 1, 5, 1, 4]), np.array([5, 6, 5, 3, 6]), c)  # pos_a == pos_b
    assert "positions" in refused(a, np.array([5, 7, 5, 3, 6]), c)                          # out of range
    assert "positions" in refused(np.array([3, -1, 0, 1, 4]), b, c)
    assert "positions" in refused(a, b, c, n=6, part=part[:6])
    assert "takes no part" in refused(np.array([2, 1, 0, 1, 4]), b, c)
    assert "min_clusters 0" in refused(a, b, c, K=0)
    assert "threshold is NaN" in refused(a, b, c, thr=float("nan"))
    lib = _ffi.lib()
    assert lib.pcv_linkage_cut(None, None, None, 3, None, 7, 0.5, 1, None, None) == PCV_ERR_INVALID
    assert lib.pcv_linkage_cut(None, None, None, 0, None, 7, 0.5, 1, None, None) == PCV_ERR_INVALID  # out_label
    assert lib.pcv_linkage_cut(None, None, None, -1, None, 0, 0.5, 1, None, None) == PCV_ERR_INVALID
    equal_c = np.array([0.9, 0.8, 0.8, 0.1, 0.1])  # equal weights are in order
    assert pa.linkage_cut(a, b, equal_c, 7, part, 0.8)[1] == 3


def test_cut_at_a_threshold_is_the_density_reference_at_min_items_1(oracle):
    rng = np.random.default_rng(21)
    centres = rng.standard_normal((6, 24))
    rows = (centres[rng.integers(0, 6, size=300)] + 0.45 * rng.standard_normal((300, 24))).astype(np.float32)
    rows[17] = 0.0
    rows[101, 3] = np.inf
    part = np.ones(300, dtype=bool)
    part[[5, 250]] = False
    ids = np.arange(300, dtype=np.int64) + 9000
    _ids, tp, pos_a, pos_b, _ia, _ib, c = reference(oracle, rows, ids, part)
    assert tp.sum() == 296
    live = np.nonzero(tp)[0]
    seen = set()
    for thr in (0.3, 0.6, 0.9, float(np.float32(c[len(c) // 2])), float(np.nextafter(np.float32(1.0), np.float32(0.0)))):
        t = float(np.float32(thr))
        pairs = density_ref.near_pairs(oracle, rows, thr, live)
        labels, _kinds, _degrees, clusters = density_ref.cluster(300, live, [(a, b) for a, b, _c in pairs], 1)
        got = pa.linkage_cut(pos_a, pos_b, c, 300, tp, t)
        assert got[0].tolist() == labels.tolist() and got[1] == clusters
        assert cut(300, tp, (pos_a, pos_b, c), t)[0].tolist() == labels.tolist()
        seen.add(clusters)
    assert len(seen) >= 3  # (the thresholds cut the corpus at different heights)
