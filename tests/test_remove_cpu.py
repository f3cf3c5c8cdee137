"""CPU: removed items (pcv_searcher_remove_ids) are declared, exported, bound and present in the regenerated Rust ffi; the
argument checks need no GPU; the Python, C++ and Rust surfaces reach the entry point."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import perceive_amd as pa
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
NEW = ("pcv_searcher_remove_ids",)


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
    assert ("pub fn pcv_searcher_remove_ids(s: *mut pcv_searcher, ids: *const i64, n: i64, out_rows: *mut i64) -> c_int;"
            in ffi_rs)


def test_bad_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    ids = np.arange(4, dtype=np.int64)
    n = C.c_int64()
    fake = C.c_void_p(1)  # never dereferenced: the argument checks come first
    assert lib.pcv_searcher_remove_ids(None, _ffi.i64p(ids), 4, C.byref(n)) == PCV_ERR_INVALID
    assert "NULL" in lib.pcv_last_error().decode()
    assert lib.pcv_searcher_remove_ids(None, _ffi.i64p(ids), -1, None) == PCV_ERR_INVALID
    assert lib.pcv_searcher_remove_ids(fake, _ffi.i64p(ids), -1, None) == PCV_ERR_INVALID
    assert lib.pcv_searcher_remove_ids(fake, None, 4, None) == PCV_ERR_INVALID
    assert "NULL" in lib.pcv_last_error().decode()


def test_python_surface():
    assert callable(getattr(pa.Searcher, "remove_items"))
    assert callable(getattr(pa.search.SearcherView, "remove_items"))  # (inherited: the library refuses it on a view)


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn remove_items\(&mut self, ids: &\[i64\]\) -> Result<usize, HipError>(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::remove_items"
    assert "ffi::pcv_searcher_remove_ids(" in m.group(1)
    doc = search_rs[: m.start()].rsplit("\n\n", 1)[-1]  # its comment names where the reference does this by rebuilding
    assert "search.rs:58-79" in doc and "cmd/source.rs" in doc and "rebuild_search" in doc


def test_cpp_mirror_remove_program_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "remove_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "remove_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)
