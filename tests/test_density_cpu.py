"""CPU: density clusters (pcv_searcher_density_clusters, pcv_searcher_last_density_stats) are declared, exported, bound and present
in the regenerated Rust ffi; the argument checks need no GPU; the Python, C++ and Rust surfaces reach the call; and the reference
the GPU tests compare with (density_ref.py) gives the answers written out here by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import perceive_amd as pa
from density_ref import BORDER, CORE, NOISE, NONE, cluster, margin, reference, takes_part
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
ARITY = {"pcv_searcher_density_clusters": 12, "pcv_searcher_last_density_stats": 2}
STATS = ["rows", "participating", "sure_pairs", "candidates", "confirmed", "core", "border", "noise", "clusters", "tile_rows", "reruns",
         "prep_ms", "degree_ms", "rescore_ms", "link_ms", "label_ms"]


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
    m = re.search(r"\bpcv_searcher_density_clusters\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "pcv_searcher* s", "const int64_t* source_ids", "int n_sources", "float threshold", "int min_items", "int64_t capacity",
        "int64_t* out_ids", "int32_t* out_label", "int8_t* out_kind", "int32_t* out_degree", "int64_t* out_rows", "int32_t* out_clusters"]
    m = re.search(r"enum\s*\{\s*PCV_DENSITY_NONE\s*=\s*-1,\s*PCV_DENSITY_NOISE\s*=\s*0,\s*PCV_DENSITY_BORDER\s*=\s*1,\s*PCV_DENSITY_CORE\s*=\s*2\s*\}", header)
    assert m
    from perceive_amd import search

    for mod in (search, pa):
        assert (mod.PCV_DENSITY_NONE, mod.PCV_DENSITY_NOISE, mod.PCV_DENSITY_BORDER, mod.PCV_DENSITY_CORE) == (-1, 0, 1, 2)
    assert (NONE, NOISE, BORDER, CORE) == (-1, 0, 1, 2)
    # the stats struct: the header's fields, in order, with the binding's widths
    m = re.search(r"typedef struct pcv_density_stats \{(.*?)\} pcv_density_stats;", header, flags=re.S)
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, widths[t]) for n, t in fields] == list(_ffi.DensityStats._fields_)
    assert [n for n, _ in fields] == STATS
    assert [t for _, t in fields] == ["int64_t"] * 8 + ["int32_t"] * 3 + ["float"] * 5
    assert C.sizeof(_ffi.DensityStats) == 96


def test_regenerated_rust_ffi_is_current():
    path = os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")
    ffi_rs = open(path).read()
    assert ("pub fn pcv_searcher_density_clusters(s: *mut pcv_searcher, source_ids: *const i64, n_sources: c_int, threshold: f32, "
            "min_items: c_int, capacity: i64, out_ids: *mut i64, out_label: *mut i32, out_kind: *mut int8_t, out_degree: *mut i32, "
            "out_rows: *mut i64, out_clusters: *mut i32) -> c_int;") in ffi_rs
    assert "pub type int8_t = i8;" in ffi_rs
    assert "pub fn pcv_searcher_last_density_stats(s: *mut pcv_searcher, out: *mut pcv_density_stats) -> c_int;" in ffi_rs
    for name, value in (("NONE", -1), ("NOISE", 0), ("BORDER", 1), ("CORE", 2)):
        assert "pub const PCV_DENSITY_%s: c_int = %d;" % (name, value) in ffi_rs
    want = r"pub struct pcv_density_stats \{\s*" + r"\s*".join(
        r"pub %s: %s," % (n, "i64" if i < 8 else "i32" if i < 11 else "f32") for i, n in enumerate(STATS)) + r"\s*\}"
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
    ids = np.full(4, -77, dtype=np.int64)
    label = np.full(4, -77, dtype=np.int32)
    kind = np.full(4, -77, dtype=np.int8)
    degree = np.full(4, -77, dtype=np.int32)
    rows = C.c_int64(-5)
    clusters = C.c_int32(-5)
    arrays = dict(ids_p=_ffi.i64p(ids), label_p=_ffi.i32p(label), kind_p=_ffi.i8p(kind), degree_p=_ffi.i32p(degree), clusters_p=C.byref(clusters))
    nothing = dict(ids_p=None, label_p=None, kind_p=None, degree_p=None, clusters_p=None)

    def call(s, threshold=0.9, min_items=3, capacity=4, rows_p=C.byref(rows), **kw):
        a = dict(arrays, **kw)
        return lib.pcv_searcher_density_clusters(s, None, 0, threshold, min_items, capacity, a["ids_p"], a["label_p"], a["kind_p"], a["degree_p"],
                                                 rows_p, a["clusters_p"])

    def message():
        msg = lib.pcv_last_error().decode()
        assert "density_clusters" in msg
        return msg

    assert call(None) == PCV_ERR_INVALID
    assert "searcher is NULL" in message()
    assert call(None, capacity=0, **nothing) == PCV_ERR_INVALID  # counting only, too
    assert "searcher is NULL" in message()
    assert call(fake, rows_p=None) == PCV_ERR_INVALID
    assert "out_rows is NULL" in message()
    assert call(fake, threshold=float("nan")) == PCV_ERR_INVALID
    assert "threshold is NaN" in message()
    for thr in (-1.0, -1.5, float(np.nextafter(np.float32(1.0), np.float32(2.0))), 2.0, float("inf"), float("-inf")):
        assert call(fake, threshold=thr) == PCV_ERR_INVALID
        assert "outside (-1, 1]" in message()
        assert call(fake, threshold=thr, capacity=0, **nothing) == PCV_ERR_INVALID
    for m in (0, -1, -(1 << 31)):
        assert call(fake, min_items=m) == PCV_ERR_INVALID
        assert "min_items %d is below 1" % m in message()
    for cap in (-1, -(1 << 40)):
        assert call(fake, capacity=cap) == PCV_ERR_INVALID
        assert "capacity %d is negative" % cap in message()
    for name in ("label_p", "kind_p", "clusters_p"):  # (out_ids and out_degree may be NULL)
        assert call(fake, **{name: None}) == PCV_ERR_INVALID
        assert "is NULL with capacity 4" in message()
    assert call(fake, capacity=4, **nothing) == PCV_ERR_INVALID  # counting only means capacity 0
    assert call(fake, capacity=0, **dict(nothing, ids_p=arrays["ids_p"])) == PCV_ERR_INVALID  # ... and every array NULL
    assert call(fake, capacity=0, **dict(nothing, degree_p=arrays["degree_p"])) == PCV_ERR_INVALID
    assert rows.value == -5 and clusters.value == -5  # nothing was written
    assert (ids == -77).all() and (label == -77).all() and (kind == -77).all() and (degree == -77).all()
    st = _ffi.DensityStats()
    assert lib.pcv_searcher_last_density_stats(None, C.byref(st)) == PCV_ERR_INVALID
    assert lib.pcv_searcher_last_density_stats(fake, None) == PCV_ERR_INVALID
    assert b"last_density_stats" in lib.pcv_last_error()


def test_python_surface():
    for cls in (pa.Searcher, pa.SearcherView):
        for name in ("density_clusters", "last_density_stats"):
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("density_clusters", "last_density_stats"):
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited
    src = open(os.path.join(ROOT, "perceive_amd", "search.py")).read()
    body = src[src.index("    def density_clusters("):src.index("    def last_density_stats(")]
    assert body.count("pcv_searcher_density_clusters(") == 2  # the count, then the clusters


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn density_clusters\(&self,\s*sources: &\[i64\],\s*threshold: f32,\s*min_items: usize\) -> \(Vec<\(i64, i32, i8, i32\)>, usize\)(.*?)\n    }\n",
                  search_rs, flags=re.S)
    assert m, "Searcher::density_clusters"
    assert m.group(1).count("ffi::pcv_searcher_density_clusters(") == 2
    assert search_rs.index("pub fn density_clusters(") < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_density_program_compiles():
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count(" density_clusters(") == 2 and hpp.count("pcv_searcher_density_clusters(") == 2  # Searcher and SearcherView; the count, then the clusters
    assert hpp.count(" last_density_stats(") == 2
    src = os.path.join(ROOT, "tests", "cpp", "density_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "density_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


# ---- the reference against answers written out by hand ----------------------------------------------------------------------------
def plane_rows(degrees, dim=8, seed=3):
    """rows in one plane of a dim-d space at the given angles, of several lengths: the cosine of two is cos(angle difference)"""
    rng = np.random.default_rng(seed)
    t = np.deg2rad(np.asarray(degrees, dtype=np.float64))
    rows = np.zeros((len(degrees), dim))
    rows[:, 2] = np.cos(t)
    rows[:, 5] = np.sin(t)
    return np.ascontiguousarray((rows * rng.uniform(0.5, 2.0, size=(len(degrees), 1))).astype(np.float32))


THR = float(np.float32(np.cos(np.deg2rad(10.0))))  # near: within 10 degrees; every angle difference below is at least 1 degree off


def test_the_graph_rules_on_a_hand_made_graph():
    # positions 0..7; 7 takes no part.  Edges: a triangle 1-2-4, a path 4-5, 0-3, 3-6
    live = [0, 1, 2, 3, 4, 5, 6]
    pairs = [(1, 2), (2, 4), (1, 4), (4, 5), (0, 3), (3, 6)]
    labels, kinds, degrees, clusters = cluster(8, live, pairs, 3)
    # core: degree >= 2: rows 1, 2, 4 (one component) and 3 (alone).  Row 1 comes before row 3: clusters 0 and 1
    assert degrees.tolist() == [1, 2, 2, 2, 3, 1, 1, 0]
    assert kinds.tolist() == [BORDER, CORE, CORE, CORE, CORE, BORDER, BORDER, NONE]
    assert labels.tolist() == [1, 0, 0, 1, 0, 0, 1, -1] and clusters == 2
    labels, kinds, degrees, clusters = cluster(8, live, pairs, 1)  # every participating row is core: the components
    assert kinds.tolist() == [CORE] * 7 + [NONE] and labels.tolist() == [0, 1, 1, 0, 1, 1, 0, -1] and clusters == 2
    labels, kinds, degrees, clusters = cluster(8, live, pairs, 4)  # only row 4 is core
    assert kinds.tolist() == [NOISE, BORDER, BORDER, NOISE, CORE, BORDER, NOISE, NONE]
    assert labels.tolist() == [-1, 0, 0, -1, 0, 0, -1, -1] and clusters == 1


def test_a_border_row_near_two_clusters_goes_to_the_lower_position(oracle):
    """A: 0, 3, 6, 8 degrees; B: 26, 28, 31, 34; the row at 17 is within 10 degrees of A's row at 8 and of B's row at 26 and of nothing
    else.  min_items 4: the eight are core (three partners each in their own group), the row at 17 (two partners) is not.  B's row
    at 26 is stored first: B is cluster 0, and the border row, near positions 0 and 4, takes position 0's label."""
    angles = [26, 0, 3, 6, 8, 17, 28, 31, 34, 120]
    rows = plane_rows(angles)
    ids = np.arange(10, dtype=np.int64) * 11 + 5
    got = reference(oracle, rows, ids, THR, 4)
    assert got[0].tolist() == ids.tolist()
    assert got[3].tolist() == [4, 3, 3, 3, 4, 2, 3, 3, 3, 0]
    assert got[2].tolist() == [CORE] * 5 + [BORDER] + [CORE] * 3 + [NOISE]
    assert got[1].tolist() == [0, 1, 1, 1, 1, 0, 0, 0, 0, -1] and got[4] == 2
    assert sorted((a, b) for a, b, _c in reference.pairs) == sorted(
        [(1, 2), (1, 3), (1, 4), (2, 3), (2, 4), (3, 4), (4, 5), (0, 5), (0, 6), (0, 7), (0, 8), (6, 7), (6, 8), (7, 8)])
    # min_items 3: the row at 17 is core too and joins the two groups
    got = reference(oracle, rows, ids, THR, 3)
    assert got[2].tolist() == [CORE] * 9 + [NOISE] and got[1].tolist() == [0] * 9 + [-1] and got[4] == 1
    # with A stored first the border row goes to A
    order = [1, 2, 3, 4, 0, 5, 6, 7, 8, 9]
    got = reference(oracle, rows[order], ids[order], THR, 4)
    assert got[1].tolist() == [0, 0, 0, 0, 1, 0, 1, 1, 1, -1] and got[2][5] == BORDER


def test_min_items_above_the_row_count_and_rows_without_a_part(oracle):
    angles = [26, 0, 3, 6, 8, 17, 28, 31, 34, 120]
    rows = plane_rows(angles)
    ids = np.arange(10, dtype=np.int64)
    got = reference(oracle, rows, ids, THR, 11)
    assert got[1].tolist() == [-1] * 10 and got[2].tolist() == [NOISE] * 10 and got[4] == 0
    assert got[3].tolist() == [4, 3, 3, 3, 4, 2, 3, 3, 3, 0]  # the degrees do not depend on min_items
    # a zero row, a row with a NaN and a hidden row take no part: kind -1, degree 0, and their partners lose them
    rows2 = rows.copy()
    rows2[2] = 0.0
    rows2[7, 1] = np.nan
    part = np.ones(10, dtype=bool)
    part[0] = False
    assert takes_part(rows2, part).tolist() == [False, True, False, True, True, True, True, False, True, True]
    got = reference(oracle, rows2, ids, THR, 1)
    assert got[2].tolist() == [CORE, CORE, NONE, CORE, CORE, CORE, CORE, NONE, CORE, CORE]  # (nothing hidden in this call)
    got = reference(oracle, rows2, ids, THR, 1, part)
    assert got[2].tolist() == [NONE, CORE, NONE, CORE, CORE, CORE, CORE, NONE, CORE, CORE]
    assert got[3].tolist() == [0, 2, 0, 2, 3, 1, 1, 0, 1, 0]
    # 1, 3, 4, 5 hang together (0-6-8-17); 28 and 34 are 6 apart; 120 is alone: a cluster of one at min_items 1
    assert got[1].tolist() == [-1, 0, -1, 0, 0, 0, 1, -1, 1, 2] and got[4] == 3


def test_margin_is_the_library_formula():
    # selfjoin_margin(Dp): 0.00783 + 1.02 (Dp + 16) 1.2e-7 + 1e-6
    assert abs(margin(384) - (0.00783 + 1.02 * 400 * 1.2e-7 + 1e-6)) < 1e-9
    assert margin(100) == margin(112) and margin(64) < margin(384) < 0.0079
