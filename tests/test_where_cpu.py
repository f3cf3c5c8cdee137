"""CPU: item values and filtered search (pcv_searcher_set_values ... pcv_searcher_create_view_where) are declared, exported, bound
and present in the regenerated Rust ffi; the argument checks need no GPU; the Python, C++ and Rust surfaces reach the calls; and the
reference walk of tests/where_ref.py does what the definition says on a list small enough to check by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import grouped_ref
import perceive_amd as pa
import where_ref
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
PCV_MAX_RESULTS = 128
PCV_MAX_WHERE_POOL = 4096
PCV_NO_VALUE = -(1 << 63)
PCV_WHERE_UNSET_PASSES, PCV_WHERE_OUTSIDE = 1, 2
ARGS = {
    "pcv_searcher_set_values": 4,
    "pcv_searcher_clear_values": 1,
    "pcv_searcher_get_values": 4,
    "pcv_searcher_value_stats": 2,
    "pcv_searcher_count_where": 8,
    "pcv_searcher_search_where": 16,
    "pcv_searcher_create_view_where": 5,
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
    m = re.search(r"enum\s*\{\s*PCV_MAX_WHERE_POOL\s*=\s*(\d+)\s*\}", header)
    assert m and int(m.group(1)) == PCV_MAX_WHERE_POOL
    assert re.search(r"#define\s+PCV_NO_VALUE\s+\(INT64_MIN\)", header)
    m = re.search(r"enum\s*\{\s*PCV_WHERE_UNSET_PASSES\s*=\s*(\d+)\s*,\s*PCV_WHERE_OUTSIDE\s*=\s*(\d+)\s*\}", header)
    assert m and (int(m.group(1)), int(m.group(2))) == (PCV_WHERE_UNSET_PASSES, PCV_WHERE_OUTSIDE)
    from perceive_amd import search

    assert search.PCV_MAX_WHERE_POOL == PCV_MAX_WHERE_POOL and search.PCV_NO_VALUE == PCV_NO_VALUE == np.iinfo(np.int64).min
    assert (search.WHERE_UNSET_PASSES, search.WHERE_OUTSIDE) == (PCV_WHERE_UNSET_PASSES, PCV_WHERE_OUTSIDE)
    assert (pa.WHERE_UNSET_PASSES, pa.WHERE_OUTSIDE, pa.PCV_NO_VALUE) == (PCV_WHERE_UNSET_PASSES, PCV_WHERE_OUTSIDE, PCV_NO_VALUE)
    assert where_ref.NO_VALUE == PCV_NO_VALUE and (where_ref.UNSET_PASSES, where_ref.OUTSIDE) == (PCV_WHERE_UNSET_PASSES, PCV_WHERE_OUTSIDE)
    assert where_ref.default_pool is grouped_ref.default_pool and where_ref.default_pool(10) == 128 and where_ref.default_pool(128) == 1024
    # the stats struct: the header's fields, in order, with their widths — those of pcv_group_stats
    m = re.search(r"typedef struct pcv_value_stats \{(.*?)\} pcv_value_stats;", header, flags=re.S)
    fields = [tuple(d.split()) for d in m.group(1).split(";") if d.strip()]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, widths[t]) for t, n in fields] == list(_ffi.ValueStats._fields_) == list(_ffi.GroupStats._fields_)
    assert [n for _t, n in fields] == ["ids", "entries", "slots", "rehashes", "last_set_ms"]
    assert C.sizeof(_ffi.ValueStats) == 32


def test_regenerated_rust_ffi_is_current():
    path = os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")
    ffi_rs = open(path).read()
    for decl in (
        "pub fn pcv_searcher_set_values(s: *mut pcv_searcher, ids: *const i64, values: *const i64, n: i64) -> c_int;",
        "pub fn pcv_searcher_clear_values(s: *mut pcv_searcher) -> c_int;",
        "pub fn pcv_searcher_get_values(s: *mut pcv_searcher, ids: *const i64, n: i64, out_values: *mut i64) -> c_int;",
        "pub fn pcv_searcher_value_stats(s: *mut pcv_searcher, out: *mut pcv_value_stats) -> c_int;",
        "pub fn pcv_searcher_count_where(s: *mut pcv_searcher, source_ids: *const i64, n_sources: c_int, lo: i64, hi: i64, flags: u32, "
        "out_rows: *mut i64, out_searchable: *mut i64) -> c_int;",
        "pub fn pcv_searcher_search_where(s: *mut pcv_searcher, queries: *const f32, n_queries: c_int, source_ids: *const i64, "
        "n_sources: c_int, num_results: c_int, pool: c_int, lo: i64, hi: i64, flags: u32, out_ids: *mut i64, out_scores: *mut f32, "
        "out_values: *mut i64, out_counts: *mut i32, out_examined: *mut i32, out_more: *mut u8) -> c_int;",
        "pub fn pcv_searcher_create_view_where(parent: *mut pcv_searcher, lo: i64, hi: i64, flags: u32, "
        "out_view: *mut *mut pcv_searcher) -> c_int;",
        "pub const PCV_MAX_WHERE_POOL: c_int = %d;" % PCV_MAX_WHERE_POOL,
        "pub const PCV_WHERE_UNSET_PASSES: c_int = %d;" % PCV_WHERE_UNSET_PASSES,
        "pub const PCV_WHERE_OUTSIDE: c_int = %d;" % PCV_WHERE_OUTSIDE,
        "pub const PCV_NO_VALUE: i64 = i64::MIN;",
    ):
        assert decl in ffi_rs, decl
    assert re.search(r"pub struct pcv_value_stats \{\s*pub ids: i64,\s*pub entries: i64,\s*pub slots: i64,\s*pub rehashes: i32,\s*"
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


def message(who):
    msg = _ffi.lib().pcv_last_error().decode()
    assert who + ": " in msg, msg
    return msg


def test_bad_search_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    fake = C.c_void_p(1)  # never dereferenced: the argument checks come first
    q = np.zeros((2, 8), dtype=np.float32)
    ids = np.zeros((2, 4), dtype=np.int64)
    cnt = np.zeros(2, dtype=np.int32)

    def call(s, q_p, nq, k=4, pool=128, flags=0):
        return lib.pcv_searcher_search_where(s, q_p, nq, None, 0, k, pool, 0, 10, flags, _ffi.i64p(ids), None, None, _ffi.i32p(cnt), None, None)

    assert call(None, _ffi.f32p(q), 2) == PCV_ERR_INVALID
    assert "search_where: searcher is NULL" in message("search_where")
    assert call(fake, None, 2) == PCV_ERR_INVALID
    assert "search_where: no queries" in message("search_where")
    for nq in (0, -3):
        assert call(fake, _ffi.f32p(q), nq) == PCV_ERR_INVALID
        assert "search_where: no queries" in message("search_where")
    for k in (0, -1, PCV_MAX_RESULTS + 1, 1 << 20):
        assert call(fake, _ffi.f32p(q), 2, k=k, pool=PCV_MAX_WHERE_POOL) == PCV_ERR_INVALID
        assert "search_where: num_results %d outside [1,%d]" % (k, PCV_MAX_RESULTS) in message("search_where")
    for k, pool in ((4, 3), (4, 0), (4, -5), (4, PCV_MAX_WHERE_POOL + 1), (128, 127)):
        assert call(fake, _ffi.f32p(q), 2, k=k, pool=pool) == PCV_ERR_INVALID
        assert "search_where: pool %d outside" % pool in message("search_where")
    for flags in (4, 8, 1 << 31, 3 | 16):
        assert call(fake, _ffi.f32p(q), 2, flags=flags) == PCV_ERR_INVALID
        assert "search_where: unknown flag bits in %#x" % flags in message("search_where")


def test_bad_table_count_and_view_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    fake = C.c_void_p(1)  # never dereferenced: the argument checks come first
    ids = np.array([5, 6, 7], dtype=np.int64)
    out = np.zeros(3, dtype=np.int64)
    good = np.array([0, PCV_NO_VALUE, np.iinfo(np.int64).max], dtype=np.int64)  # (every int64 is legal)
    assert lib.pcv_searcher_set_values(None, _ffi.i64p(ids), _ffi.i64p(good), 3) == PCV_ERR_INVALID
    assert "searcher is NULL" in message("set_values")
    assert lib.pcv_searcher_set_values(fake, None, _ffi.i64p(good), 3) == PCV_ERR_INVALID
    assert "NULL with n > 0" in message("set_values")
    assert lib.pcv_searcher_set_values(fake, _ffi.i64p(ids), None, 3) == PCV_ERR_INVALID
    assert "NULL with n > 0" in message("set_values")
    assert lib.pcv_searcher_set_values(fake, _ffi.i64p(ids), _ffi.i64p(good), -1) == PCV_ERR_INVALID
    assert "n < 0" in message("set_values")
    assert lib.pcv_searcher_clear_values(None) == PCV_ERR_INVALID
    assert "searcher is NULL" in message("clear_values")
    assert lib.pcv_searcher_get_values(None, _ffi.i64p(ids), 3, _ffi.i64p(out)) == PCV_ERR_INVALID
    assert "searcher is NULL" in message("get_values")
    assert lib.pcv_searcher_get_values(fake, None, 3, _ffi.i64p(out)) == PCV_ERR_INVALID
    assert "NULL with n > 0" in message("get_values")
    assert lib.pcv_searcher_get_values(fake, _ffi.i64p(ids), 3, None) == PCV_ERR_INVALID
    assert "NULL with n > 0" in message("get_values")
    assert lib.pcv_searcher_get_values(fake, _ffi.i64p(ids), -2, _ffi.i64p(out)) == PCV_ERR_INVALID
    assert "n < 0" in message("get_values")
    assert lib.pcv_searcher_value_stats(None, C.byref(_ffi.ValueStats())) == PCV_ERR_INVALID
    assert "NULL argument" in message("value_stats")
    assert lib.pcv_searcher_value_stats(fake, None) == PCV_ERR_INVALID
    assert "NULL argument" in message("value_stats")
    rows, live = C.c_int64(), C.c_int64()
    assert lib.pcv_searcher_count_where(None, None, 0, 0, 10, 0, C.byref(rows), C.byref(live)) == PCV_ERR_INVALID
    assert "searcher is NULL" in message("count_where")
    assert lib.pcv_searcher_count_where(fake, None, 2, 0, 10, 0, C.byref(rows), C.byref(live)) == PCV_ERR_INVALID
    assert "NULL with n_sources > 0" in message("count_where")
    assert lib.pcv_searcher_count_where(fake, _ffi.i64p(ids), -1, 0, 10, 0, C.byref(rows), C.byref(live)) == PCV_ERR_INVALID
    assert "n_sources < 0" in message("count_where")
    for flags in (4, 1 << 30, 7):
        assert lib.pcv_searcher_count_where(fake, None, 0, 0, 10, flags, C.byref(rows), C.byref(live)) == PCV_ERR_INVALID
        assert "count_where: unknown flag bits in %#x" % flags in message("count_where")
    h = C.c_void_p(77)
    assert lib.pcv_searcher_create_view_where(None, 0, 10, 0, C.byref(h)) == PCV_ERR_INVALID
    assert "NULL argument" in message("create_view_where")
    assert lib.pcv_searcher_create_view_where(fake, 0, 10, 0, None) == PCV_ERR_INVALID
    assert "NULL argument" in message("create_view_where")
    for flags in (4, 255):
        h = C.c_void_p(77)
        assert lib.pcv_searcher_create_view_where(fake, 0, 10, flags, C.byref(h)) == PCV_ERR_INVALID
        assert "create_view_where: unknown flag bits in %#x" % flags in message("create_view_where")
        assert not h.value  # (the out pointer is cleared before anything can fail)


def test_python_surface():
    names = ("set_values", "clear_values", "values_of", "value_stats", "count_where", "search_where", "search_where_vector",
             "search_where_like_item", "view_where")
    for cls in (pa.Searcher, pa.SearcherView):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    for name in names[:-1]:
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited
    assert pa.SearcherView.view_where is not pa.Searcher.view_where  # (a view refuses to be a parent, as with view)


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn search_vector_where\(\s*&self,\s*sources: &\[i64\],\s*num_results: usize,\s*vector: Vec<f32>,\s*lo: i64,\s*hi: i64,\s*"
                  r"flags: u32,\s*pool: Option<usize>,?\s*\) -> Vec<\(SearchItem, i64\)>(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::search_vector_where"
    assert "ffi::pcv_searcher_search_where(" in m.group(1) and "ffi::PCV_MAX_WHERE_POOL" in m.group(1) and "ffi::PCV_NO_VALUE" in m.group(1)
    m = re.search(r"pub fn set_values\(&mut self, ids: &\[i64\], values: &\[i64\]\)(.*?)\n    }\n", search_rs, flags=re.S)
    assert m and "ffi::pcv_searcher_set_values(" in m.group(1)
    m = re.search(r"pub fn view_where\(&self, lo: i64, hi: i64, flags: u32\) -> Result<SearcherView<'_>, HipError>(.*?)\n    }\n", search_rs, flags=re.S)
    assert m and "ffi::pcv_searcher_create_view_where(" in m.group(1)
    for fn in ("pub fn search_vector_where(", "pub fn set_values(", "pub fn view_where("):
        assert search_rs.index(fn) < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_where_program_compiles():
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count("search_vector_where(") == 2 and "pcv_searcher_search_where(" in hpp  # Searcher and SearcherView
    assert hpp.count("int64_t count_where(") == 2 and "pcv_searcher_count_where(" in hpp
    for call in ("pcv_searcher_set_values(", "pcv_searcher_clear_values(", "pcv_searcher_get_values(", "pcv_searcher_value_stats(",
                 "pcv_searcher_create_view_where("):
        assert call in hpp
    src = os.path.join(ROOT, "tests", "cpp", "where_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "where_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


def test_reference_walk_on_a_hand_made_list():
    # eight rows, best first; rows 3 and 4 tie (the list has the lower position first).  Values: row r has 10 * r, but rows 1 and 6
    # have none.
    L = [0, 1, 2, 3, 4, 5, 6, 7]
    scores = [0.9, 0.8, 0.7, 0.6, 0.6, 0.5, 0.4, 0.3]
    value = {0: 0, 2: 20, 3: 30, 4: 40, 5: 50, 7: 70}
    NONE = where_ref.NO_VALUE
    U, O = where_ref.UNSET_PASSES, where_ref.OUTSIDE

    def walk(k, pool, lo, hi, flags=0):
        return where_ref.walk_list(L, scores, value.get, k, pool, lo, hi, flags)

    # the whole list under [20, 50]: rows 2, 3, 4, 5
    assert walk(8, 8, 20, 50) == ([2, 3, 4, 5], [0.7, 0.6, 0.6, 0.5], [20, 30, 40, 50], 8, False)
    # the walk stops right after the k-th kept row: row 4 is kept third, and rows 5 .. 7 behind it are not examined
    assert walk(3, 8, 20, 50) == ([2, 3, 4], [0.7, 0.6, 0.6], [20, 30, 40], 5, False)
    assert walk(1, 8, 20, 50) == ([2], [0.7], [20], 3, False)
    # the interval is closed at both ends
    assert walk(8, 8, 21, 49)[0] == [3, 4] and walk(8, 8, 30, 30)[0] == [3]
    # a pool shorter than the list: examined == pool, fewer than k kept, and the list had more
    assert walk(4, 3, 20, 50) == ([2], [0.7], [20], 3, True)
    # ... and one that the k-th kept row ends first, or that is the whole list: no `more`
    assert walk(1, 3, 20, 50) == ([2], [0.7], [20], 3, False)
    assert walk(8, 100, 20, 50)[3:] == (8, False)
    # lo > hi keeps nothing, whatever the values; with UNSET_PASSES only the rows without a value
    assert walk(8, 8, 50, 20) == ([], [], [], 8, False)
    assert walk(8, 5, 50, 20) == ([], [], [], 5, True)
    assert walk(8, 8, 50, 20, U) == ([1, 6], [0.8, 0.4], [NONE, NONE], 8, False)
    # OUTSIDE negates the interval for the rows that have a value; the rows without one follow bit 0 alone
    assert walk(8, 8, 20, 50, O) == ([0, 7], [0.9, 0.3], [0, 70], 8, False)
    assert walk(8, 8, 20, 50, O | U) == ([0, 1, 6, 7], [0.9, 0.8, 0.4, 0.3], [0, NONE, NONE, 70], 8, False)
    assert walk(8, 8, 20, 50, U) == ([1, 2, 3, 4, 5, 6], [0.8, 0.7, 0.6, 0.6, 0.5, 0.4], [NONE, 20, 30, 40, 50, NONE], 8, False)
    assert walk(8, 8, 50, 20, O)[0] == [0, 2, 3, 4, 5, 7]  # outside the empty interval: every row with a value
    assert walk(2, 8, 20, 50, O | U) == ([0, 1], [0.9, 0.8], [0, NONE], 2, False)
    # an entry that holds NO_VALUE is no value
    assert where_ref.passes(NONE, NONE, np.iinfo(np.int64).max, 0) is False and where_ref.passes(NONE + 1, NONE, NONE + 1, 0) is True
    assert where_ref.count([1, 2, 3, 3], {1: 5, 2: NONE, 3: 7}, 5, 7, 0) == 3 and where_ref.count([1, 2, 3, 3], {1: 5, 2: NONE, 3: 7}, 6, 9, O | U) == 2

    # the values follow the ids: WhereReference looks the value up by id
    class FakeOracle:
        def topk(self, queries, rows, k, metric=0):
            n = rows.shape[0]
            return np.arange(n)[None, :], np.linspace(0.9, 0.1, n)[None, :], np.array([n])

    ids = np.array([50, 50, 60, 60, 70], dtype=np.int64)
    ref = where_ref.WhereReference(FakeOracle(), np.zeros((1, 4), np.float32), np.zeros((5, 4), np.float32), ids, "cosine")
    w = ref.walk(0, 5, 128, {50: 3, 70: 9}, 0, 5)
    assert w[0].tolist() == [50, 50] and w[2].tolist() == [3, 3] and w[3:] == (5, False)
    w = ref.walk(0, 5, 128, {50: 3, 60: NONE}, 0, 5, U, allowed=np.array([1, 2, 3]))
    assert w[0].tolist() == [50, 60, 60] and w[2].tolist() == [3, NONE, NONE] and w[3] == 3
    np.testing.assert_array_equal(w[1].view(np.uint32), np.linspace(0.9, 0.1, 5)[1:4].astype(np.float32).view(np.uint32))
