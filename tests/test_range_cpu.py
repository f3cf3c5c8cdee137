"""CPU: range search (pcv_searcher_search_range) is declared, exported, bound and present in the regenerated Rust ffi; the
argument checks need no GPU; the Python, C++ and Rust surfaces reach the call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import perceive_amd as pa
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
NAME = "pcv_searcher_search_range"
PCV_MAX_RANGE_ROWS = 1 << 24


def test_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "perceive_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pcv_[a-z0-9_]+)", out))
    lib = _ffi.lib()
    assert re.search(r"\b%s\s*\(" % NAME, header)
    assert NAME in exported
    assert NAME in _ffi.SYMBOLS and getattr(lib, NAME).argtypes
    assert len(_ffi.SYMBOLS[NAME][1]) == 11
    m = re.search(r"enum\s*\{\s*PCV_MAX_RANGE_ROWS\s*=\s*(\d+)\s*\}", header)
    assert m and int(m.group(1)) == PCV_MAX_RANGE_ROWS


def test_regenerated_rust_ffi_is_current():
    path = os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")
    ffi_rs = open(path).read()
    assert ("pub fn pcv_searcher_search_range(s: *mut pcv_searcher, queries: *const f32, n_queries: c_int, source_ids: *const i64, "
            "n_sources: c_int, bounds: *const f32, max_results: i64, out_ids: *mut i64, out_scores: *mut f32, out_counts: *mut i64, "
            "out_more: *mut u8) -> c_int;") in ffi_rs
    assert "pub const PCV_MAX_RANGE_ROWS: c_int = %d;" % PCV_MAX_RANGE_ROWS in ffi_rs
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
    q = np.zeros((2, 8), dtype=np.float32)
    b = np.array([0.5, 0.25], dtype=np.float32)
    ids = np.zeros((2, 4), dtype=np.int64)
    cnt = np.zeros(2, dtype=np.int64)

    def call(s, q_p, nq, b_p, m):
        return lib.pcv_searcher_search_range(s, q_p, nq, None, 0, b_p, m, _ffi.i64p(ids), None, _ffi.i64p(cnt), None)

    def message():
        msg = lib.pcv_last_error().decode()
        assert "search_range" in msg
        return msg

    assert call(None, _ffi.f32p(q), 2, _ffi.f32p(b), 4) == PCV_ERR_INVALID
    assert "searcher is NULL" in message()
    assert call(fake, None, 2, _ffi.f32p(b), 4) == PCV_ERR_INVALID
    assert "no queries" in message()
    for nq in (0, -3):
        assert call(fake, _ffi.f32p(q), nq, _ffi.f32p(b), 4) == PCV_ERR_INVALID
        assert "no queries" in message()
    assert call(fake, _ffi.f32p(q), 2, None, 4) == PCV_ERR_INVALID
    assert "bounds is NULL" in message()
    nan = np.array([0.5, np.nan], dtype=np.float32)
    assert call(fake, _ffi.f32p(q), 2, _ffi.f32p(nan), 4) == PCV_ERR_INVALID
    assert "query 1 is NaN" in message()
    for m in (0, -1, PCV_MAX_RANGE_ROWS + 1, 1 << 40):
        assert call(fake, _ffi.f32p(q), 2, _ffi.f32p(b), m) == PCV_ERR_INVALID
        assert "max_results" in message()


def test_python_surface():
    for cls in (pa.Searcher, pa.SearcherView):
        for name in ("search_range", "search_range_vector", "search_range_like_item"):
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("search_range", "search_range_vector", "search_range_like_item"):
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn search_vector_range\(&self, sources: &\[i64\], bound: f32, max_results: usize, vector: Vec<f32>\) -> "
                  r"\(Vec<SearchItem>, bool\)(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::search_vector_range"
    assert "ffi::pcv_searcher_search_range(" in m.group(1)
    assert search_rs.index("pub fn search_vector_range(") < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_range_program_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "range_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "range_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


def test_mirrors_agree_on_room_for_nothing():
    """max_results == 0 is PCV_ERR_INVALID at the C ABI; the C++ and Rust mirrors both answer it with an empty result instead"""
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    assert "if (sources.empty() || max_results == 0) return {};" in hpp
    assert "if self.handle.is_null() || max_results == 0 {\n            return (Vec::new(), false);" in search_rs
