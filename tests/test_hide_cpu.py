"""CPU: hidden items (pcv_searcher_hide_ids / _unhide_ids / _hidden_ids) are declared, exported and bound; their argument checks
need no GPU; the Rust shim and the C++ mirror reach them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import perceive_amd as pa
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
NEW = ("pcv_searcher_hide_ids", "pcv_searcher_unhide_ids", "pcv_searcher_hidden_ids")


def test_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "perceive_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pcv_[a-z0-9_]+)", out))
    lib = _ffi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported, name
        assert name in _ffi.SYMBOLS and getattr(lib, name).argtypes, name


def test_bad_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    ids = np.arange(4, dtype=np.int64)
    rows, n = C.c_int64(), C.c_int64()
    for fn in (lib.pcv_searcher_hide_ids, lib.pcv_searcher_unhide_ids):
        assert fn(None, _ffi.i64p(ids), 4, C.byref(rows)) == PCV_ERR_INVALID
        assert fn(None, _ffi.i64p(ids), -1, C.byref(rows)) == PCV_ERR_INVALID
        assert "NULL" in lib.pcv_last_error().decode()
    assert lib.pcv_searcher_hidden_ids(None, None, 0, C.byref(n), None) == PCV_ERR_INVALID
    assert lib.pcv_searcher_hidden_ids(None, None, -1, C.byref(n), None) == PCV_ERR_INVALID


def test_python_surface():
    for name in ("hide_items", "unhide_items", "hidden_items"):
        assert callable(getattr(pa.Searcher, name))
        assert callable(getattr(pa.ShardedSearcher, name))
    assert isinstance(pa.Searcher.hidden_rows, property)


def test_rust_shim_declares_and_calls_them():
    ffi_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")).read()
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    for name in NEW:
        assert re.search(r"pub fn %s\(" % name, ffi_rs), name
    hide = re.search(r"pub fn hide_items\(&mut self, ids: &\[i64\]\)(.*?)\n    }\n", search_rs, flags=re.S)
    unhide = re.search(r"pub fn unhide_items\(&mut self, ids: &\[i64\]\)(.*?)\n    }\n", search_rs, flags=re.S)
    assert hide and "ffi::pcv_searcher_hide_ids(" in hide.group(1) and "self.hidden" in hide.group(1)
    assert unhide and "ffi::pcv_searcher_unhide_ids(" in unhide.group(1) and "self.hidden" in unhide.group(1)
    assert "pub hidden: HashSet<i64>" in search_rs


def test_cpp_mirror_hide_program_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "hide_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "hide_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)
