"""CPU: the reach tree (pcv_searcher_reach_tree, pcv_searcher_last_reach_stats) and pcv_linkage_select are declared, exported, bound
and present in the regenerated Rust ffi and the C++ mirror; the argument checks that come before the handle need no GPU;
pcv_linkage_select, which needs none at all, agrees with the selection written in plain Python (reach_ref.select) and with results
written out here by hand; and the reference the GPU tests compare with (reach_ref.reference) gives the trees written out by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
import linkage_ref
from perceive_amd import _ffi
from reach_ref import bits, check_select, reference, select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
ARITY = {"pcv_searcher_reach_tree": 16, "pcv_searcher_last_reach_stats": 2, "pcv_linkage_select": 13}
STATS = ["rows", "participating", "edges", "core_candidates", "candidates", "rounds", "tile_rows", "reruns", "min_items", "core_ms", "prep_ms",
         "bound_ms", "list_ms", "rescore_ms", "merge_ms"]


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
    m = re.search(r"\bpcv_searcher_reach_tree\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "pcv_searcher* s", "const int64_t* source_ids", "int n_sources", "int min_items", "int64_t capacity", "int64_t* out_ids",
        "int8_t* out_part", "double* out_core", "int64_t* out_pos_a", "int64_t* out_pos_b", "int64_t* out_id_a", "int64_t* out_id_b",
        "double* out_w", "double* out_c", "int64_t* out_rows", "int64_t* out_edges"]
    m = re.search(r"\bpcv_linkage_select\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "const int64_t* pos_a", "const int64_t* pos_b", "const double* w", "int64_t n_edges", "const int8_t* part", "int64_t n_rows",
        "int64_t min_cluster_size", "int allow_single", "int32_t* out_label", "int32_t* out_clusters", "double* out_stability",
        "int64_t* out_size", "int64_t cluster_capacity"]
    m = re.search(r"typedef struct pcv_reach_stats \{(.*?)\} pcv_reach_stats;", header, flags=re.S)
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, widths[t]) for n, t in fields] == list(_ffi.ReachStats._fields_)
    assert [n for n, _ in fields] == STATS
    assert [t for _, t in fields] == ["int64_t"] * 5 + ["int32_t"] * 4 + ["float"] * 6
    assert C.sizeof(_ffi.ReachStats) == 80


def test_python_cpp_and_rust_surfaces():
    for name in ("reach_tree", "last_reach_stats"):
        assert callable(getattr(pa.Searcher, name))
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited
    assert callable(pa.linkage_select)
    src = open(os.path.join(ROOT, "perceive_amd", "search.py")).read()
    body = src[src.index("    def reach_tree("):src.index("    def last_reach_stats(")]
    assert body.count("pcv_searcher_reach_tree(") == 2  # the count, then the tree
    ffi_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")).read()
    assert ("pub fn pcv_searcher_reach_tree(s: *mut pcv_searcher, source_ids: *const i64, n_sources: c_int, min_items: c_int, capacity: i64, "
            "out_ids: *mut i64, out_part: *mut int8_t, out_core: *mut f64, out_pos_a: *mut i64, out_pos_b: *mut i64, out_id_a: *mut i64, "
            "out_id_b: *mut i64, out_w: *mut f64, out_c: *mut f64, out_rows: *mut i64, out_edges: *mut i64) -> c_int;") in ffi_rs
    assert "pub fn pcv_searcher_last_reach_stats(s: *mut pcv_searcher, out: *mut pcv_reach_stats) -> c_int;" in ffi_rs
    assert ("pub fn pcv_linkage_select(pos_a: *const i64, pos_b: *const i64, w: *const f64, n_edges: i64, part: *const int8_t, n_rows: i64, "
            "min_cluster_size: i64, allow_single: c_int, out_label: *mut i32, out_clusters: *mut i32, out_stability: *mut f64, "
            "out_size: *mut i64, cluster_capacity: i64) -> c_int;") in ffi_rs
    want = r"pub struct pcv_reach_stats \{\s*" + r"\s*".join(
        r"pub %s: %s," % (n, "i64" if i < 5 else "i32" if i < 9 else "f32") for i, n in enumerate(STATS)) + r"\s*\}"
    assert re.search(want, ffi_rs)
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn reach_tree\(&self,\s*sources: &\[i64\], min_items: usize\) -> \(Vec<\(i64, bool, f64\)>, Vec<\(i64, i64, f64\)>\)(.*?)\n    }\n",
                  search_rs, flags=re.S)
    assert m, "Searcher::reach_tree"
    assert m.group(1).count("ffi::pcv_searcher_reach_tree(") == 2
    assert search_rs.index("pub fn reach_tree(") < search_rs.index("impl Drop for Searcher")
    assert re.search(r"\npub fn linkage_select\(", search_rs) and search_rs.count("ffi::pcv_linkage_select(") == 1
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count(" reach_tree(") == 2 and hpp.count("pcv_searcher_reach_tree(") == 2  # Searcher and SearcherView; the count, then the tree
    assert hpp.count(" last_reach_stats(") == 2 and hpp.count("inline LinkageSelection linkage_select(") == 3
    # the host file of the selection is compiled without contraction, and says so where the compiler reads it
    sel = open(os.path.join(ROOT, "perceive_amd", "csrc", "linkage_select.cpp")).read()
    assert "#pragma clang fp contract(off)" in sel and sel.index("#pragma clang fp contract(off)") < sel.index("pcv_status pcv_linkage_select(")


def test_cpp_mirror_reach_program_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "reach_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "reach_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


def test_bad_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    fake = C.c_void_p(1)  # never dereferenced: the argument checks come first
    i64 = {k: np.full(4, -77, dtype=np.int64) for k in ("ids", "pos_a", "pos_b", "id_a", "id_b")}
    f64 = {k: np.full(4, -77.0, dtype=np.float64) for k in ("core", "w", "c")}
    part = np.full(4, -77, dtype=np.int8)
    rows, edges = C.c_int64(-5), C.c_int64(-5)
    arrays = dict({k + "_p": _ffi.i64p(v) for k, v in i64.items()}, part_p=_ffi.i8p(part), edges_p=C.byref(edges),
                  **{k + "_p": _ffi.f64p(v) for k, v in f64.items()})
    nothing = {k: None for k in arrays}

    def call(s, min_items=5, capacity=4, rows_p=C.byref(rows), **kw):
        a = dict(arrays, **kw)
        return lib.pcv_searcher_reach_tree(s, None, 0, min_items, capacity, a["ids_p"], a["part_p"], a["core_p"], a["pos_a_p"], a["pos_b_p"],
                                           a["id_a_p"], a["id_b_p"], a["w_p"], a["c_p"], rows_p, a["edges_p"])

    def message():
        msg = lib.pcv_last_error().decode()
        assert "reach_tree" in msg
        return msg

    assert call(None) == PCV_ERR_INVALID
    assert "searcher is NULL" in message()
    assert call(None, capacity=0, **nothing) == PCV_ERR_INVALID  # the n-only form, too
    assert "searcher is NULL" in message()
    assert call(fake, rows_p=None) == PCV_ERR_INVALID
    assert "out_rows is NULL" in message()
    for mi in (0, -1, 66, 1 << 20):  # min_items outside 1 .. PCV_MAX_NEIGHBORS + 1: before the handle is looked at
        assert call(fake, min_items=mi) == PCV_ERR_INVALID
        assert "min_items %d outside [1,65]" % mi in message()
        assert call(fake, min_items=mi, capacity=0, **nothing) == PCV_ERR_INVALID
    for cap in (-1, -(1 << 40)):
        assert call(fake, capacity=cap) == PCV_ERR_INVALID
        assert "capacity %d is negative" % cap in message()
    for name in ("pos_a_p", "pos_b_p", "w_p", "edges_p"):  # (out_ids, out_part, out_core, out_c and the edges' ids may be NULL)
        assert call(fake, **{name: None}) == PCV_ERR_INVALID
        assert "is NULL with capacity 4" in message()
    for name in ("id_a_p", "id_b_p"):  # ... the edges' ids both or neither
        assert call(fake, **{name: None}) == PCV_ERR_INVALID
        assert "one of out_id_a and out_id_b" in message()
    assert call(fake, capacity=4, **nothing) == PCV_ERR_INVALID  # the n-only form means capacity 0
    for name in ("ids_p", "part_p", "core_p", "id_a_p", "c_p", "w_p"):  # ... and every array NULL
        assert call(fake, capacity=0, **dict(nothing, **{name: arrays[name]})) == PCV_ERR_INVALID
    assert rows.value == -5 and edges.value == -5  # nothing was written
    assert all((v == -77).all() for v in i64.values()) and (part == -77).all() and all((v == -77.0).all() for v in f64.values())
    st = _ffi.ReachStats()
    assert lib.pcv_searcher_last_reach_stats(None, C.byref(st)) == PCV_ERR_INVALID
    assert lib.pcv_searcher_last_reach_stats(fake, None) == PCV_ERR_INVALID
    assert b"last_reach_stats" in lib.pcv_last_error()


def test_no_gpu_fails_loudly():
    """reach_tree is a device entry point: without a device there is no context to build a searcher in, and no quiet way round it
    (test_abi.py); with one, this test has nothing to say."""
    if pa.device_count() == 0:
        with pytest.raises(pa.PcvError) as e:
            pa.Context(0)
        assert e.value.status == 2 and "no HIP device" in str(e.value)


# ---- the reference against trees written out by hand ------------------------------------------------------------------------------
def plane_rows(degrees, dim=8, seed=3):
    """test_linkage_cpu.py's: rows in one plane at the given angles, of several lengths; the cosine of two is cos(angle difference)"""
    rng = np.random.default_rng(seed)
    t = np.deg2rad(np.asarray(degrees, dtype=np.float64))
    rows = np.zeros((len(degrees), dim))
    rows[:, 2] = np.cos(t)
    rows[:, 5] = np.sin(t)
    return np.ascontiguousarray((rows * rng.uniform(0.5, 2.0, size=(len(degrees), 1))).astype(np.float32))


def test_reference_three_tight_rows_and_a_stray(oracle):
    """A, B, C at 0, 3 and 6 degrees, the stray S at 8: two degrees from C, five from B, eight from A.  Single linkage takes (C, S)
    first.  At min_items = 3 a core is a row's second best c:
        core(A) = c(A, C) (6)   core(B) = min(c(A, B), c(B, C)) (3)   core(C) = c(B, C) (3; S is C's best)   core(S) = c(B, S) (5)
        w(B, C) = core(B)                    the best edge
        w(C, S) = w(B, S) = c(B, S)          S's low core caps its edge with C at 5 degrees: it sinks behind (B, C), ties with (B, S),
                                             and the lower position wins the tie — S hangs on B, not on its nearest row
        w(A, B) = w(A, C) = c(A, C)          tie again: (A, B)
        w(A, S) = c(A, S)"""
    rows = plane_rows([0, 3, 6, 8])
    ids = np.array([50, 40, 30, 20], dtype=np.int64)
    c = lambda a, b: oracle.canonical_score(rows[a], rows[b], 0)
    assert c(2, 3) > max(c(0, 1), c(1, 2)) > min(c(0, 1), c(1, 2)) > c(1, 3) > c(0, 2) > c(0, 3)
    plain = linkage_ref.reference(oracle, rows, ids)
    assert (plain[2][0], plain[3][0]) == (2, 3) and sorted(zip(plain[2][1:].tolist(), plain[3][1:].tolist())) == [(0, 1), (1, 2)]
    got = reference(oracle, rows, ids, 3)
    assert got[0].tolist() == ids.tolist() and got[1].tolist() == [1, 1, 1, 1]
    assert got[2].tolist() == [c(0, 2), min(c(0, 1), c(1, 2)), c(1, 2), c(1, 3)]                        # core
    assert list(zip(got[3].tolist(), got[4].tolist())) == [(1, 2), (1, 3), (0, 1)]
    assert got[5].tolist() == [40, 40, 50] and got[6].tolist() == [30, 20, 40]
    assert got[7].tolist() == [min(c(0, 1), c(1, 2)), c(1, 3), c(0, 2)]                                 # w
    assert got[8].tolist() == [c(1, 2), c(1, 3), c(0, 1)]                                               # c
    # min_items = 1 is the linkage tree, w == c; min_items = 2 caps with the best partner, which changes no weight's order here
    one = reference(oracle, rows, ids, 1)
    assert (one[2] == np.inf).all()
    for k, j in ((3, 2), (4, 3), (7, 6)):
        np.testing.assert_array_equal(one[k], plain[j])
    np.testing.assert_array_equal(bits(one[7]), bits(plain[6]))
    np.testing.assert_array_equal(bits(one[8]), bits(plain[6]))
    # more items than rows: j = P - 1 = 3, every core is the row's worst c, and a row that takes no part changes P
    big = reference(oracle, rows, ids, 65)
    assert big[2].tolist() == [c(0, 3), c(1, 3), c(0, 2), c(0, 3)]
    rows2 = rows.copy()
    rows2[1] = 0.0
    out = reference(oracle, rows2, ids, 3)
    assert out[1].tolist() == [1, 0, 1, 1] and np.isnan(out[2][1])
    assert out[2][[0, 2, 3]].tolist() == [c(0, 3), c(0, 2), c(0, 3)]  # j = 2 = P - 1
    assert list(zip(out[3].tolist(), out[4].tolist())) == [(0, 2), (0, 3)] and out[7].tolist() == [c(0, 3), c(0, 3)]


def star_rows():
    return np.ascontiguousarray(np.eye(64, dtype=np.float32)[:, ::-1] * np.float32(3.0))  # 64 orthonormal directions, every c exactly 0


@pytest.mark.parametrize("min_items", [1, 3, 65])
def test_reference_on_the_star(oracle, min_items):
    """Every c is exactly 0, so every core is (or +inf) and every w: the positions alone order the edges."""
    got = reference(oracle, star_rows(), np.arange(64, dtype=np.int64), min_items)
    assert got[3].tolist() == [0] * 63 and got[4].tolist() == list(range(1, 64))
    assert (got[7] == 0.0).all() and (got[8] == 0.0).all() and (got[2] == (np.inf if min_items == 1 else 0.0)).all()


# ---- pcv_linkage_select against the plain Python, and against results written out by hand -----------------------------------------
def line_tree(x):
    """the single-linkage tree of points on a line under w = 1 - |x_a - x_b| / 64 (exact for the dyadic x used here), in the edge order"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    a, b = np.triu_indices(n, 1)
    w = 1.0 - np.abs(x[a] - x[b]) / 64.0
    order = np.lexsort((b, a, -w))
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v

    tree = []
    for i in order:
        p, q = find(int(a[i])), find(int(b[i]))
        if p != q:
            parent[max(p, q)] = min(p, q)
            tree.append((int(a[i]), int(b[i]), float(w[i])))
    return (np.array([t[0] for t in tree], dtype=np.int64), np.array([t[1] for t in tree], dtype=np.int64),
            np.array([t[2] for t in tree], dtype=np.float64))


def both(n, part, edges, M, allow_single=False):
    got = pa.linkage_select(edges[0], edges[1], edges[2], n, part, M, allow_single)
    check_select(got, select(n, part, edges, M, allow_single))
    return got


def test_select_two_blobs_and_noise():
    rng = np.random.default_rng(5)
    blob1 = rng.integers(0, 256, size=25) / 256.0          # in [0, 1)
    blob2 = 4.0 + rng.integers(0, 256, size=30) / 256.0    # in [4, 5)
    noise = np.array([-20.0, 30.0, 47.0, -41.0])           # farther from everything than the blobs are from each other
    x = np.concatenate([blob1, blob2, noise])
    perm = rng.permutation(len(x))
    x = x[perm]
    kind = np.concatenate([np.zeros(25), np.ones(30), np.full(4, 2)])[perm].astype(int)
    edges = line_tree(x)
    labels, stab, size = both(len(x), None, edges, 5)
    assert (labels[kind == 2] == -1).all() and len(stab) == 2 and sorted(size.tolist()) == [25, 30]
    assert len(set(labels[kind == 0].tolist())) == 1 and len(set(labels[kind == 1].tolist())) == 1 and labels[kind == 0][0] != labels[kind == 1][0]
    assert labels[np.nonzero(kind != 2)[0][0]] == 0  # numbered by the lowest position
    assert (stab > 0).all()
    # with the root allowed it wins: 55 rows stay in it from its birth (a gap of 25) to the split (a gap of about 3), which is more
    # than the blobs gain afterwards — and the noise rows, which left the root, are its rows
    labels1, stab1, size1 = both(len(x), None, edges, 5, True)
    assert (labels1 == 0).all() and size1.tolist() == [len(x)] and stab1[0] > stab.sum()
    # rows that take no part keep their place and get -1
    part = np.ones(len(x) + 3, dtype=np.int8)
    part[[0, 7, len(x) + 2]] = 0
    live = np.nonzero(part)[0]
    e2 = (live[edges[0]], live[edges[1]], edges[2])
    lo, hi = np.minimum(e2[0], e2[1]), np.maximum(e2[0], e2[1])
    labels2, stab2, size2 = both(len(part), part, (lo, hi, e2[2]), 5)
    np.testing.assert_array_equal(labels2[live], labels)
    assert (labels2[part == 0] == -1).all() and bits(stab2).tolist() == bits(stab).tolist()


def test_select_one_blob():
    """x_i = 2^i / 2^20: every gap is larger than all the gaps before it together, so the tree peels one row off the far end at a
    time and no node has two children of min_cluster_size rows: the root is the only cluster."""
    x = [2.0 ** i / 2.0 ** 20 for i in range(24)]
    edges = line_tree(x)
    assert edges[0].tolist() == list(range(23)) and edges[1].tolist() == list(range(1, 24))
    labels, stab, size = both(24, None, edges, 5, False)
    assert (labels == -1).all() and len(stab) == 0
    labels, stab, size = both(24, None, edges, 5, True)
    assert (labels == 0).all() and size.tolist() == [24] and stab[0] > 0


def test_select_tie_goes_to_the_parent():
    """Rows 0..3 are the cluster C: born at 0 (the root splits at once into C and the pair D = {4, 5}), it splits at 0.25 into the
    pairs {0, 1} and {2, 3}, which fall apart at 0.5.  S(C) = 4 (0.25 - 0) = 1, S of each pair = 2 (0.5 - 0.25) = 0.5: a tie, and
    the parent wins it.  Every number is a dyadic fraction: the tie is exact."""
    edges = (np.array([0, 2, 4, 0, 0]), np.array([1, 3, 5, 2, 4]), np.array([0.5, 0.5, 0.5, 0.25, 0.0]))
    labels, stab, size = both(6, None, edges, 2)
    assert labels.tolist() == [0, 0, 0, 0, 1, 1] and stab.tolist() == [1.0, 1.0] and size.tolist() == [4, 2]
    # a hair more for the children and they win
    edges2 = (edges[0], edges[1], np.array([0.5 + 2.0 ** -40, 0.5, 0.5, 0.25, 0.0]))
    labels, stab, size = both(6, None, edges2, 2)
    assert labels.tolist() == [0, 0, 1, 1, 2, 2] and size.tolist() == [2, 2, 2]
    # the root is a candidate only when asked: S(root) = 0 < 2, so it loses all the same
    assert both(6, None, edges, 2, True)[0].tolist() == [0, 0, 0, 0, 1, 1]


def test_select_min_cluster_size_above_the_rows():
    edges = (np.array([0, 2, 4, 0, 0]), np.array([1, 3, 5, 2, 4]), np.array([0.5, 0.5, 0.5, 0.25, 0.0]))
    labels, stab, size = both(6, None, edges, 10)
    assert (labels == -1).all() and len(stab) == 0 and len(size) == 0
    # the root's cluster is there all the same, of stability 0 (every row leaves it where it is born): asked for, it is the answer
    labels, stab, size = both(6, None, edges, 10, True)
    assert (labels == 0).all() and stab.tolist() == [0.0] and size.tolist() == [6]
    # no edges: one row, and none
    for n in (1, 0):
        e = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
        labels, stab, size = both(n, None, e, 2, True)
        assert (labels == -1).all() and len(labels) == n and len(stab) == 0


def test_select_random_trees_agree():
    rng = np.random.default_rng(11)
    for n in (2, 3, 17, 200):
        for M in (2, 3, 8):
            x = rng.integers(0, 1 << 12, size=n) / 64.0  # many equal gaps: ties in w
            edges = line_tree(x)
            for single in (False, True):
                both(n, None, edges, M, single)


def test_select_on_a_linkage_tree(oracle):
    rng = np.random.default_rng(13)
    centres = rng.standard_normal((3, 32))
    rows = np.ascontiguousarray((centres[rng.integers(0, 3, size=90)] + 0.3 * rng.standard_normal((90, 32))).astype(np.float32))
    rows[17] = 0.0
    ids = np.arange(90, dtype=np.int64)
    t = linkage_ref.reference(oracle, rows, ids)
    labels, stab, size = both(90, t[1], (t[2], t[3], t[6]), 6)
    assert labels[17] == -1 and len(stab) == 3 and size.sum() >= 60
    r = reference(oracle, rows, ids, 4)
    labels, stab, size = both(90, r[1], (r[3], r[4], r[7]), 6)
    assert labels[17] == -1 and len(stab) == 3


def test_select_argument_and_order_errors():
    lib = _ffi.lib()
    a = np.array([0, 2, 0], dtype=np.int64)
    b = np.array([1, 3, 2], dtype=np.int64)
    w = np.array([0.9, 0.8, 0.1], dtype=np.float64)
    part = np.ones(4, dtype=np.int8)
    labels = np.full(4, -77, dtype=np.int32)
    k = C.c_int32(-5)

    def call(a=a, b=b, w=w, n_edges=3, part=part, n_rows=4, M=2, labels=labels, cap=0):
        return lib.pcv_linkage_select(_ffi.i64p(a), _ffi.i64p(b), _ffi.f64p(w), n_edges, None if part is None else _ffi.i8p(part), n_rows, M, 0,
                                      None if labels is None else _ffi.i32p(labels), C.byref(k), None, None, cap)

    def refused(text, **kw):
        assert call(**kw) == PCV_ERR_INVALID
        msg = lib.pcv_last_error().decode()
        assert "linkage_select" in msg and text in msg, msg

    assert call() == 0 and k.value == 2 and labels.tolist() == [0, 0, 1, 1]
    assert call(part=None) == 0
    for M in (1, 0, -3):
        refused("min_cluster_size %d is below 2" % M, M=M)
    refused("not ordered from best to worst at edge 1", w=np.array([0.8, 0.9, 0.1]))
    refused("not ordered from best to worst at edge 2", w=np.array([0.9, 0.8, np.nan]))
    refused("joins positions 1 and 0", a=np.array([1, 2, 0], dtype=np.int64), b=np.array([0, 3, 2], dtype=np.int64))
    refused("joins positions 2 and 2", b=np.array([1, 2, 2], dtype=np.int64))
    refused("joins positions 2 and 4", b=np.array([1, 4, 2], dtype=np.int64))
    refused("joins positions -1 and 1", a=np.array([-1, 2, 0], dtype=np.int64))
    refused("3 edges do not span 3 participating rows", part=np.array([1, 1, 1, 0], dtype=np.int8))
    refused("2 edges do not span 4 participating rows", n_edges=2)
    refused("closes a cycle", a=np.array([0, 0, 2], dtype=np.int64), b=np.array([1, 1, 3], dtype=np.int64))
    refused("has an end that takes no part", part=np.array([1, 1, 0, 1, 1], dtype=np.int8), n_rows=5)
    refused("out_label is NULL", labels=None)
    refused("-1 edges", n_edges=-1)
    refused("cluster_capacity 3 without an array", cap=3)
    refused("cluster_capacity -1 is negative", cap=-1)
    with pytest.raises(ValueError):
        pa.linkage_select(a, b, w[:2], 4)
    with pytest.raises(ValueError):
        pa.linkage_select(a, b, w, 4, part[:3])
    with pytest.raises(pa.PcvError) as e:
        pa.linkage_select(a, b, w, 4, None, 1)
    assert e.value.status == PCV_ERR_INVALID
