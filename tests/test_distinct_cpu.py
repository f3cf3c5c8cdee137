"""CPU: distinct results (pcv_searcher_search_distinct) are declared, exported, bound and present in the regenerated Rust ffi; the
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
NAME = "pcv_searcher_search_distinct"
PCV_MAX_RESULTS = 128
PCV_MAX_DISTINCT_POOL = 4096


def test_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "perceive_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pcv_[a-z0-9_]+)", out))
    lib = _ffi.lib()
    assert re.search(r"\b%s\s*\(" % NAME, header)
    assert NAME in exported
    assert NAME in _ffi.SYMBOLS and getattr(lib, NAME).argtypes
    assert len(_ffi.SYMBOLS[NAME][1]) == 14
    m = re.search(r"enum\s*\{\s*PCV_MAX_DISTINCT_POOL\s*=\s*(\d+)\s*\}", header)
    assert m and int(m.group(1)) == PCV_MAX_DISTINCT_POOL
    from perceive_amd import search

    assert search.PCV_MAX_DISTINCT_POOL == PCV_MAX_DISTINCT_POOL


def test_regenerated_rust_ffi_is_current():
    path = os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")
    ffi_rs = open(path).read()
    assert ("pub fn pcv_searcher_search_distinct(s: *mut pcv_searcher, queries: *const f32, n_queries: c_int, source_ids: *const i64, "
            "n_sources: c_int, num_results: c_int, threshold: f32, pool: c_int, out_ids: *mut i64, out_scores: *mut f32, "
            "out_counts: *mut i32, out_similar: *mut i32, out_examined: *mut i32, out_more: *mut u8) -> c_int;") in ffi_rs
    assert "pub const PCV_MAX_DISTINCT_POOL: c_int = %d;" % PCV_MAX_DISTINCT_POOL in ffi_rs
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
    ids = np.zeros((2, 4), dtype=np.int64)
    cnt = np.zeros(2, dtype=np.int32)

    def call(s, q_p, nq, k=4, threshold=0.9, pool=128):
        return lib.pcv_searcher_search_distinct(s, q_p, nq, None, 0, k, threshold, pool, _ffi.i64p(ids), None, _ffi.i32p(cnt), None, None, None)

    def message():
        msg = lib.pcv_last_error().decode()
        assert "search_distinct" in msg
        return msg

    assert call(None, _ffi.f32p(q), 2) == PCV_ERR_INVALID
    assert "searcher is NULL" in message()
    assert call(fake, None, 2) == PCV_ERR_INVALID
    assert "no queries" in message()
    for nq in (0, -3):
        assert call(fake, _ffi.f32p(q), nq) == PCV_ERR_INVALID
        assert "no queries" in message()
    for k in (0, -1, PCV_MAX_RESULTS + 1, 1 << 20):
        assert call(fake, _ffi.f32p(q), 2, k=k, pool=PCV_MAX_DISTINCT_POOL) == PCV_ERR_INVALID
        assert "num_results %d outside [1,%d]" % (k, PCV_MAX_RESULTS) in message()
    for k, pool in ((4, 3), (4, 0), (4, -5), (4, PCV_MAX_DISTINCT_POOL + 1), (128, 127)):
        assert call(fake, _ffi.f32p(q), 2, k=k, pool=pool) == PCV_ERR_INVALID
        assert "pool %d outside" % pool in message()
    for t in (float("nan"),):
        assert call(fake, _ffi.f32p(q), 2, threshold=t) == PCV_ERR_INVALID
        assert "threshold is NaN" in message()
    for t in (-1.0, -2.5, float(np.nextafter(np.float32(1.0), np.float32(2.0))), 3.0, float("inf"), float("-inf")):
        assert call(fake, _ffi.f32p(q), 2, threshold=t) == PCV_ERR_INVALID
        assert "threshold" in message() and "outside (-1, 1]" in message()


def test_python_surface():
    names = ("search_distinct", "search_distinct_vector", "search_distinct_like_item")
    for cls in (pa.Searcher, pa.SearcherView):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    for name in names:
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn search_vector_distinct\(\s*&self,\s*sources: &\[i64\],\s*num_results: usize,\s*vector: Vec<f32>,\s*threshold: f32,\s*"
                  r"pool: Option<usize>,?\s*\) -> Vec<\(SearchItem, i32\)>(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::search_vector_distinct"
    assert "ffi::pcv_searcher_search_distinct(" in m.group(1) and "ffi::PCV_MAX_DISTINCT_POOL" in m.group(1)
    assert search_rs.index("pub fn search_vector_distinct(") < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_distinct_program_compiles():
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count("search_vector_distinct(") == 2 and "pcv_searcher_search_distinct(" in hpp  # Searcher and SearcherView
    src = os.path.join(ROOT, "tests", "cpp", "distinct_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "distinct_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)
