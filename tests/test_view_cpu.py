"""CPU: views (pcv_searcher_create_view / _view_stats) are declared, exported, bound and present in the regenerated Rust ffi;
their argument checks need no GPU; the Python, C++ and Rust surfaces reach them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import perceive_amd as pa
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
NEW = ("pcv_searcher_create_view", "pcv_searcher_view_stats")


def test_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "perceive_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pcv_[a-z0-9_]+)", out))
    lib = _ffi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported, name
        assert name in _ffi.SYMBOLS and getattr(lib, name).argtypes, name


def test_regenerated_rust_ffi_is_current():
    ffi_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")).read()
    assert re.search(r"pub fn pcv_searcher_create_view\(parent: \*mut pcv_searcher, ids: \*const i64, n: i64, "
                     r"out_view: \*mut \*mut pcv_searcher\) -> c_int;", ffi_rs)
    assert re.search(r"pub fn pcv_searcher_view_stats\(view: \*mut pcv_searcher, out_rows: \*mut i64, out_ids: \*mut i64, "
                     r"out_refreshes: \*mut i32, out_build_ms: \*mut f32\) -> c_int;", ffi_rs)


def test_bad_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    ids = np.arange(4, dtype=np.int64)
    out = C.c_void_p()
    fake = C.c_void_p(1)  # never dereferenced: the argument checks come first
    assert lib.pcv_searcher_create_view(None, _ffi.i64p(ids), 4, C.byref(out)) == PCV_ERR_INVALID
    assert "NULL" in lib.pcv_last_error().decode()
    assert lib.pcv_searcher_create_view(fake, _ffi.i64p(ids), 4, None) == PCV_ERR_INVALID
    assert lib.pcv_searcher_create_view(fake, None, 4, C.byref(out)) == PCV_ERR_INVALID
    assert "NULL with n > 0" in lib.pcv_last_error().decode()
    assert lib.pcv_searcher_create_view(fake, _ffi.i64p(ids), -1, C.byref(out)) == PCV_ERR_INVALID
    assert "n < 0" in lib.pcv_last_error().decode()
    assert not out.value
    assert lib.pcv_searcher_view_stats(None, None, None, None, None) == PCV_ERR_INVALID


def test_python_surface():
    assert callable(pa.Searcher.view)
    assert issubclass(pa.SearcherView, pa.Searcher)
    for name in ("view_stats", "search_vectors", "search_device", "search_device_begin", "search_sharded"):
        assert callable(getattr(pa.SearcherView, name)), name
    assert callable(pa.ShardedSearcher.view)


def test_rust_shim_declares_and_calls_them():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn view\(&self, items: &\[i64\]\) -> Result<SearcherView<'_>, HipError>(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::view"
    assert "ffi::pcv_searcher_create_view(" in m.group(1)
    impl = search_rs[search_rs.index("impl SearcherView<'_> {"):]
    assert "pub fn search_vector(&self, sources: &[i64], num_results: usize, vector: Vec<f32>) -> Vec<SearchItem>" in impl
    assert "ffi::pcv_searcher_search(" in impl and "ffi::pcv_searcher_destroy(self.handle)" in impl


def test_cpp_mirror_view_program_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "view_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "view_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)
