"""CPU: updated items (pcv_searcher_update_rows / _update_blobs) are declared, exported, bound and present in the regenerated Rust
ffi; their argument checks need no GPU; the Python, C++ and Rust surfaces reach them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import perceive_amd as pa
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
NEW = ("pcv_searcher_update_rows", "pcv_searcher_update_blobs")


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
    assert re.search(r"pub fn pcv_searcher_update_rows\(s: \*mut pcv_searcher, ids: \*const i64, rows: \*const f32, n: i64, "
                     r"out_found: \*mut u8, out_rows: \*mut i64\) -> c_int;", ffi_rs)
    assert re.search(r"pub fn pcv_searcher_update_blobs\(s: \*mut pcv_searcher, ids: \*const i64, blobs: \*const u8, n: i64, "
                     r"out_found: \*mut u8, out_rows: \*mut i64\) -> c_int;", ffi_rs)


def test_bad_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    ids = np.arange(4, dtype=np.int64)
    rows = np.zeros((4, 8), dtype=np.float32)
    found = np.zeros(4, dtype=np.uint8)
    n = C.c_int64()
    fake = C.c_void_p(1)  # never dereferenced: the argument checks come first
    for fn, rp in ((lib.pcv_searcher_update_rows, _ffi.f32p(rows)), (lib.pcv_searcher_update_blobs, rows.ctypes.data)):
        assert fn(None, _ffi.i64p(ids), rp, 4, _ffi.u8p(found), C.byref(n)) == PCV_ERR_INVALID
        assert "NULL" in lib.pcv_last_error().decode()
        assert fn(None, _ffi.i64p(ids), rp, -1, None, None) == PCV_ERR_INVALID
        assert fn(fake, _ffi.i64p(ids), rp, -1, None, None) == PCV_ERR_INVALID
        assert fn(fake, None, rp, 4, None, None) == PCV_ERR_INVALID
        assert fn(fake, _ffi.i64p(ids), None, 4, None, None) == PCV_ERR_INVALID
        assert "NULL" in lib.pcv_last_error().decode()


def test_python_surface():
    for name in ("update_items", "update_blobs", "upsert_items"):
        assert callable(getattr(pa.Searcher, name)), name


def test_rust_shim_declares_and_calls_them():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn update_items\(&mut self, source_id: i64, items: &\[\(i64, Vec<f32>\)\]\) -> Result<\(\), HipError>"
                  r"(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::update_items"
    body = m.group(1)
    assert "ffi::pcv_searcher_update_rows(" in body
    assert "ffi::pcv_searcher_add_rows(" in body and "ffi::pcv_searcher_finalize(" in body  # upsert: unknown ids are added
    assert "cmd/source.rs" in search_rs and "rebuild_search" in search_rs


def test_cpp_mirror_update_program_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "update_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "update_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)
