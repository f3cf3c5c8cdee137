"""CPU: the group table and grouped results (pcv_searcher_set_groups ... pcv_searcher_search_grouped) are declared, exported, bound
and present in the regenerated Rust ffi; the argument checks need no GPU; the Python, C++ and Rust surfaces reach the calls; and the
reference walk of tests/grouped_ref.py does what the definition says on a list small enough to check by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import grouped_ref
import perceive_amd as pa
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
PCV_MAX_RESULTS = 128
PCV_MAX_GROUPED_POOL = 4096
PCV_NO_GROUP = -1
ARGS = {
    "pcv_searcher_set_groups": 4,
    "pcv_searcher_clear_groups": 1,
    "pcv_searcher_get_groups": 4,
    "pcv_searcher_group_stats": 2,
    "pcv_searcher_search_grouped": 14,
}


def test_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "perceive_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pcv_[a-z0-9_]+)", out))
    lib = _ffi.lib()
    for name, nargs in ARGS.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported, name
        assert name in _ffi.SYMBOLS and getattr(lib, name).argtypes, name
        assert len(_ffi.SYMBOLS[name][1]) == nargs, name
    m = re.search(r"enum\s*\{\s*PCV_MAX_GROUPED_POOL\s*=\s*(\d+)\s*\}", header)
    assert m and int(m.group(1)) == PCV_MAX_GROUPED_POOL
    m = re.search(r"#define\s+PCV_NO_GROUP\s+\((-?\d+)\)", header)
    assert m and int(m.group(1)) == PCV_NO_GROUP
    from perceive_amd import search

    assert search.PCV_MAX_GROUPED_POOL == PCV_MAX_GROUPED_POOL and search.PCV_NO_GROUP == PCV_NO_GROUP
    assert grouped_ref.NO_GROUP == PCV_NO_GROUP and grouped_ref.default_pool(10) == 128 and grouped_ref.default_pool(128) == 1024
    # the stats struct: the header's fields, in order, with their widths
    m = re.search(r"typedef struct pcv_group_stats \{(.*?)\} pcv_group_stats;", header, flags=re.S)
    fields = [tuple(d.split()) for d in m.group(1).split(";") if d.strip()]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, widths[t]) for t, n in fields] == list(_ffi.GroupStats._fields_)
    assert [n for _t, n in fields] == ["ids", "entries", "slots", "rehashes", "last_set_ms"]
    assert C.sizeof(_ffi.GroupStats) == 32


def test_regenerated_rust_ffi_is_current():
    path = os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")
    ffi_rs = open(path).read()
    for decl in (
        "pub fn pcv_searcher_set_groups(s: *mut pcv_searcher, ids: *const i64, groups: *const i64, n: i64) -> c_int;",
        "pub fn pcv_searcher_clear_groups(s: *mut pcv_searcher) -> c_int;",
        "pub fn pcv_searcher_get_groups(s: *mut pcv_searcher, ids: *const i64, n: i64, out_groups: *mut i64) -> c_int;",
        "pub fn pcv_searcher_group_stats(s: *mut pcv_searcher, out: *mut pcv_group_stats) -> c_int;",
        "pub fn pcv_searcher_search_grouped(s: *mut pcv_searcher, queries: *const f32, n_queries: c_int, source_ids: *const i64, "
        "n_sources: c_int, num_results: c_int, pool: c_int, out_ids: *mut i64, out_scores: *mut f32, out_groups: *mut i64, "
        "out_counts: *mut i32, out_collapsed: *mut i32, out_examined: *mut i32, out_more: *mut u8) -> c_int;",
        "pub const PCV_MAX_GROUPED_POOL: c_int = %d;" % PCV_MAX_GROUPED_POOL,
        "pub const PCV_NO_GROUP: i64 = %d;" % PCV_NO_GROUP,
    ):
        assert decl in ffi_rs, decl
    assert re.search(r"pub struct pcv_group_stats \{\s*pub ids: i64,\s*pub entries: i64,\s*pub slots: i64,\s*pub rehashes: i32,\s*"
                     r"pub last_set_ms: f32,\s*\}", ffi_rs)
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


def test_bad_search_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    fake = C.c_void_p(1)  # never dereferenced: the argument checks come first
    q = np.zeros((2, 8), dtype=np.float32)
    ids = np.zeros((2, 4), dtype=np.int64)
    cnt = np.zeros(2, dtype=np.int32)

    def call(s, q_p, nq, k=4, pool=128):
        return lib.pcv_searcher_search_grouped(s, q_p, nq, None, 0, k, pool, _ffi.i64p(ids), None, None, _ffi.i32p(cnt), None, None, None)

    def message():
        msg = lib.pcv_last_error().decode()
        assert "search_grouped: " in msg
        return msg

    assert call(None, _ffi.f32p(q), 2) == PCV_ERR_INVALID
    assert "search_grouped: searcher is NULL" in message()
    assert call(fake, None, 2) == PCV_ERR_INVALID
    assert "search_grouped: no queries" in message()
    for nq in (0, -3):
        assert call(fake, _ffi.f32p(q), nq) == PCV_ERR_INVALID
        assert "search_grouped: no queries" in message()
    for k in (0, -1, PCV_MAX_RESULTS + 1, 1 << 20):
        assert call(fake, _ffi.f32p(q), 2, k=k, pool=PCV_MAX_GROUPED_POOL) == PCV_ERR_INVALID
        assert "search_grouped: num_results %d outside [1,%d]" % (k, PCV_MAX_RESULTS) in message()
    for k, pool in ((4, 3), (4, 0), (4, -5), (4, PCV_MAX_GROUPED_POOL + 1), (128, 127)):
        assert call(fake, _ffi.f32p(q), 2, k=k, pool=pool) == PCV_ERR_INVALID
        assert "search_grouped: pool %d outside" % pool in message()


def test_bad_table_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    fake = C.c_void_p(1)  # never dereferenced: the argument checks come first
    ids = np.array([5, 6, 7], dtype=np.int64)
    out = np.zeros(3, dtype=np.int64)

    def message(who):
        msg = lib.pcv_last_error().decode()
        assert who + ": " in msg
        return msg

    good = np.array([0, PCV_NO_GROUP, np.iinfo(np.int64).max], dtype=np.int64)
    assert lib.pcv_searcher_set_groups(None, _ffi.i64p(ids), _ffi.i64p(good), 3) == PCV_ERR_INVALID
    assert "searcher is NULL" in message("set_groups")
    for bad in (-2, -77, np.iinfo(np.int64).min):
        groups = np.array([0, bad, 4], dtype=np.int64)
        assert lib.pcv_searcher_set_groups(fake, _ffi.i64p(ids), _ffi.i64p(groups), 3) == PCV_ERR_INVALID
        assert "group %d of id 6 (element 1)" % bad in message("set_groups")
    assert lib.pcv_searcher_set_groups(fake, None, _ffi.i64p(good), 3) == PCV_ERR_INVALID
    assert "NULL with n > 0" in message("set_groups")
    assert lib.pcv_searcher_set_groups(fake, _ffi.i64p(ids), None, 3) == PCV_ERR_INVALID
    assert "NULL with n > 0" in message("set_groups")
    assert lib.pcv_searcher_set_groups(fake, _ffi.i64p(ids), _ffi.i64p(good), -1) == PCV_ERR_INVALID
    assert "n < 0" in message("set_groups")
    assert lib.pcv_searcher_clear_groups(None) == PCV_ERR_INVALID
    assert "searcher is NULL" in message("clear_groups")
    assert lib.pcv_searcher_get_groups(None, _ffi.i64p(ids), 3, _ffi.i64p(out)) == PCV_ERR_INVALID
    assert "searcher is NULL" in message("get_groups")
    assert lib.pcv_searcher_get_groups(fake, None, 3, _ffi.i64p(out)) == PCV_ERR_INVALID
    assert "NULL with n > 0" in message("get_groups")
    assert lib.pcv_searcher_get_groups(fake, _ffi.i64p(ids), 3, None) == PCV_ERR_INVALID
    assert "NULL with n > 0" in message("get_groups")
    assert lib.pcv_searcher_group_stats(None, C.byref(_ffi.GroupStats())) == PCV_ERR_INVALID
    assert "NULL argument" in message("group_stats")
    assert lib.pcv_searcher_group_stats(fake, None) == PCV_ERR_INVALID


def test_python_surface():
    names = ("set_groups", "clear_groups", "groups_of", "group_stats", "search_grouped", "search_grouped_vector", "search_grouped_like_item")
    for cls in (pa.Searcher, pa.SearcherView):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    for name in names:
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn search_vector_grouped\(\s*&self,\s*sources: &\[i64\],\s*num_results: usize,\s*vector: Vec<f32>,\s*"
                  r"pool: Option<usize>,?\s*\) -> Vec<\(SearchItem, i64, i32\)>(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::search_vector_grouped"
    assert "ffi::pcv_searcher_search_grouped(" in m.group(1) and "ffi::PCV_MAX_GROUPED_POOL" in m.group(1) and "ffi::PCV_NO_GROUP" in m.group(1)
    m = re.search(r"pub fn set_groups\(&mut self, ids: &\[i64\], groups: &\[i64\]\)(.*?)\n    }\n", search_rs, flags=re.S)
    assert m and "ffi::pcv_searcher_set_groups(" in m.group(1)
    for fn in ("pub fn search_vector_grouped(", "pub fn set_groups("):
        assert search_rs.index(fn) < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_grouped_program_compiles():
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count("search_vector_grouped(") == 2 and "pcv_searcher_search_grouped(" in hpp  # Searcher and SearcherView
    for call in ("pcv_searcher_set_groups(", "pcv_searcher_clear_groups(", "pcv_searcher_get_groups("):
        assert call in hpp
    src = os.path.join(ROOT, "tests", "cpp", "grouped_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "grouped_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


def test_reference_walk_on_a_hand_made_list():
    # eight rows, best first; rows 3 and 4 tie (the list has the lower position first).  Group 7 = rows {0, 2, 5}: split by the
    # singleton row 1.  Group 9 = rows {4, 6}.  Rows 1, 3, 7 have no group.
    L = [0, 1, 2, 3, 4, 5, 6, 7]
    scores = [0.9, 0.8, 0.7, 0.6, 0.6, 0.5, 0.4, 0.3]
    group = {0: 7, 2: 7, 5: 7, 4: 9, 6: 9}

    def walk(k, pool):
        return grouped_ref.walk_list(L, scores, lambda r: group.get(r, -1), k, pool)

    # the whole list: four groups of their own and two shared ones
    assert walk(8, 8) == ([0, 1, 3, 4, 7], [0.9, 0.8, 0.6, 0.6, 0.3], [7, -1, -1, 9, -1], [2, 0, 0, 1, 0], 8, False)
    # the walk stops right after the k-th kept row: row 4 is kept third... fourth, and rows 5, 6 behind it are not examined
    assert walk(4, 8) == ([0, 1, 3, 4], [0.9, 0.8, 0.6, 0.6], [7, -1, -1, 9], [1, 0, 0, 0], 5, False)
    assert walk(1, 8) == ([0], [0.9], [7], [0], 1, False)
    # the tie: the lower position is walked first, whatever its group
    assert walk(3, 8)[0] == [0, 1, 3] and walk(3, 8)[4] == 4
    # a pool shorter than the list: examined == pool, fewer than k kept, and the list had more
    assert walk(4, 3) == ([0, 1], [0.9, 0.8], [7, -1], [1, 0], 3, True)
    # ... and one that the k-th kept row ends first, or that is the whole list: no `more`
    assert walk(2, 3) == ([0, 1], [0.9, 0.8], [7, -1], [0, 0], 2, False)
    assert walk(8, 100)[4:] == (8, False)
    # two rows with one id collapse iff the id has a group: GroupedReference looks the group up by id
    class FakeOracle:
        def topk(self, queries, rows, k, metric=0):
            n = rows.shape[0]
            return np.arange(n)[None, :], np.linspace(0.9, 0.1, n)[None, :], np.array([n])

    ids = np.array([50, 50, 60, 60, 70], dtype=np.int64)
    ref = grouped_ref.GroupedReference(FakeOracle(), np.zeros((1, 4), np.float32), np.zeros((5, 4), np.float32), ids, "cosine")
    w = ref.walk(0, 5, 128, {50: 3})
    assert w[0].tolist() == [50, 60, 60, 70] and w[2].tolist() == [3, -1, -1, -1] and w[3].tolist() == [1, 0, 0, 0] and w[4:] == (5, False)
    w = ref.walk(0, 5, 128, {50: 3, 60: -1}, allowed=np.array([1, 2, 3]))
    assert w[0].tolist() == [50, 60, 60] and w[3].tolist() == [0, 0, 0] and w[4] == 3
    np.testing.assert_array_equal(w[1].view(np.uint32), np.linspace(0.9, 0.1, 5)[1:4].astype(np.float32).view(np.uint32))
