"""CPU: search by example (pcv_searcher_like_queries / _search_like) is declared, exported, bound and present in the regenerated
Rust ffi; the argument checks need no GPU; the Python, C++ and Rust surfaces reach the calls."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

import perceive_amd as pa
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
NEW = ("pcv_searcher_like_queries", "pcv_searcher_search_like")


def test_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "perceive_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pcv_[a-z0-9_]+)", out))
    lib = _ffi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported, name
        assert name in _ffi.SYMBOLS and getattr(lib, name).argtypes, name
    assert len(_ffi.SYMBOLS["pcv_searcher_like_queries"][1]) == 9
    assert len(_ffi.SYMBOLS["pcv_searcher_search_like"][1]) == 13


def test_regenerated_rust_ffi_is_current():
    path = os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")
    ffi_rs = open(path).read()
    assert ("pub fn pcv_searcher_like_queries(s: *mut pcv_searcher, example_ids: *const i64, weights: *const f32, offsets: *const i64, "
            "n_queries: c_int, out_queries: *mut f32, d_out_queries: *mut c_void, out_found: *mut u8, out_member_rows: *mut i64) -> c_int;") in ffi_rs
    assert ("pub fn pcv_searcher_search_like(s: *mut pcv_searcher, example_ids: *const i64, weights: *const f32, offsets: *const i64, "
            "n_queries: c_int, source_ids: *const i64, n_sources: c_int, k: c_int, exclude_examples: c_int, out_ids: *mut i64, "
            "out_scores: *mut f32, out_counts: *mut c_int, out_found: *mut u8) -> c_int;") in ffi_rs
    # ... and the file is what the generator writes from the header today (run on a copy of the tree's two files)
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
    ids = np.arange(4, dtype=np.int64)
    ok = np.array([0, 2, 4], dtype=np.int64)
    fake = C.c_void_p(1)  # never dereferenced: the argument checks come first

    def like(s, ids_p, w_p, off_p, nq):
        return lib.pcv_searcher_like_queries(s, ids_p, w_p, off_p, nq, None, None, None, None)

    def search(s, ids_p, w_p, off_p, nq, k=10):
        return lib.pcv_searcher_search_like(s, ids_p, w_p, off_p, nq, None, 0, k, 1, None, None, None, None)

    for call, who in ((like, "like_queries"), (search, "search_like")):
        assert call(None, _ffi.i64p(ids), None, _ffi.i64p(ok), 2) == PCV_ERR_INVALID
        assert "searcher is NULL" in lib.pcv_last_error().decode() and who in lib.pcv_last_error().decode()
        assert call(fake, None, None, _ffi.i64p(ok), 2) == PCV_ERR_INVALID  # NULL ids with examples
        assert "NULL" in lib.pcv_last_error().decode()
        assert call(fake, _ffi.i64p(ids), None, None, 2) == PCV_ERR_INVALID  # NULL offsets
        assert "offsets" in lib.pcv_last_error().decode()
        bad0 = np.array([1, 2, 4], dtype=np.int64)
        assert call(fake, _ffi.i64p(ids), None, _ffi.i64p(bad0), 2) == PCV_ERR_INVALID
        assert "offsets[0]" in lib.pcv_last_error().decode()
        desc = np.array([0, 3, 2], dtype=np.int64)
        assert call(fake, _ffi.i64p(ids), None, _ffi.i64p(desc), 2) == PCV_ERR_INVALID
        assert "ascending" in lib.pcv_last_error().decode()
        assert call(fake, _ffi.i64p(ids), None, _ffi.i64p(ok), -1) == PCV_ERR_INVALID
        assert "n_queries < 0" in lib.pcv_last_error().decode()
        for bad in (np.nan, np.inf, -np.inf):
            w = np.array([1, 1, bad, 1], dtype=np.float32)
            assert call(fake, _ffi.i64p(ids), _ffi.f32p(w), _ffi.i64p(ok), 2) == PCV_ERR_INVALID
            assert "not finite" in lib.pcv_last_error().decode()
    assert search(fake, _ffi.i64p(ids), None, _ffi.i64p(ok), 2, k=0) == PCV_ERR_INVALID
    assert "num_results" in lib.pcv_last_error().decode()


def test_python_surface():
    for cls in (pa.Searcher, pa.SearcherView):
        for name in ("like_queries", "search_like", "search_like_item"):
            assert callable(getattr(cls, name)), (cls, name)
    assert pa.SearcherView.search_like is pa.Searcher.search_like  # inherited: the library looks the examples up in the parent
    ids, w, off = pa.Searcher._like_args([[5, 6], [], [7]], None)
    assert ids.tolist() == [5, 6, 7] and w is None and off.tolist() == [0, 2, 2, 3] and off.dtype == np.int64
    _, w, _ = pa.Searcher._like_args([[5, 6], [7]], [[1, -1], [0.25]])
    assert w.tolist() == [1.0, -1.0, 0.25] and w.dtype == np.float32
    _, w, _ = pa.Searcher._like_args([[5, 6], [7]], [2, 3, 4])
    assert w.tolist() == [2.0, 3.0, 4.0]
    ids, _, off = pa.Searcher._like_args([], None)
    assert ids.size == 0 and off.tolist() == [0]


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn search_like\(&self, sources: &\[i64\], num_results: usize, item_id: i64\) -> Option<Vec<SearchItem>>(.*?)\n    }\n",
                  search_rs, flags=re.S)
    assert m, "Searcher::search_like"
    assert "ffi::pcv_searcher_search_like(" in m.group(1)
    assert search_rs.index("pub fn search_like(") < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_like_program_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "like_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "like_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)
