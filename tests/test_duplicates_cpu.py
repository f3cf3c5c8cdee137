"""CPU: duplicate pairs (pcv_searcher_find_duplicates, pcv_searcher_last_duplicate_stats, pcv_duplicate_groups) are declared,
exported, bound and present in the regenerated Rust ffi; the argument checks and the grouping helper need no GPU; the Python, C++
and Rust surfaces reach the calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
PCV_MAX_DUPLICATE_PAIRS = 1 << 24
ARITY = {"pcv_searcher_find_duplicates": 10, "pcv_searcher_last_duplicate_stats": 2, "pcv_duplicate_groups": 7}


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
    m = re.search(r"enum\s*\{\s*PCV_MAX_DUPLICATE_PAIRS\s*=\s*(\d+)\s*\}", header)
    assert m and int(m.group(1)) == PCV_MAX_DUPLICATE_PAIRS
    from perceive_amd import search

    assert search.PCV_MAX_DUPLICATE_PAIRS == PCV_MAX_DUPLICATE_PAIRS
    # the stats struct: the header's fields, in order, with the binding's widths
    m = re.search(r"typedef struct pcv_duplicate_stats \{(.*?)\} pcv_duplicate_stats;", header, flags=re.S)
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, widths[t]) for n, t in fields] == list(_ffi.DuplicateStats._fields_)
    assert [n for n, _ in fields] == ["rows", "candidates", "pairs", "tile_rows", "reruns", "prep_ms", "screen_ms", "rescore_ms"]


def test_regenerated_rust_ffi_is_current():
    path = os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")
    ffi_rs = open(path).read()
    assert ("pub fn pcv_searcher_find_duplicates(s: *mut pcv_searcher, source_ids: *const i64, n_sources: c_int, threshold: f32, "
            "max_pairs: i64, out_id_a: *mut i64, out_id_b: *mut i64, out_scores: *mut f32, out_count: *mut i64, "
            "out_total: *mut i64) -> c_int;") in ffi_rs
    assert "pub fn pcv_searcher_last_duplicate_stats(s: *mut pcv_searcher, out: *mut pcv_duplicate_stats) -> c_int;" in ffi_rs
    assert ("pub fn pcv_duplicate_groups(id_a: *const i64, id_b: *const i64, n_pairs: i64, out_ids: *mut i64, out_group: *mut i64, "
            "capacity: i64, out_n_ids: *mut i64) -> c_int;") in ffi_rs
    assert "pub const PCV_MAX_DUPLICATE_PAIRS: c_int = %d;" % PCV_MAX_DUPLICATE_PAIRS in ffi_rs
    assert re.search(r"pub struct pcv_duplicate_stats \{\s*pub rows: i64,\s*pub candidates: i64,\s*pub pairs: i64,\s*pub tile_rows: i32,\s*"
                     r"pub reruns: i32,\s*pub prep_ms: f32,\s*pub screen_ms: f32,\s*pub rescore_ms: f32,\s*\}", ffi_rs)
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
    a = np.zeros(4, dtype=np.int64)
    b = np.zeros(4, dtype=np.int64)
    cnt = C.c_int64(-5)

    def call(s, a_p=_ffi.i64p(a), b_p=_ffi.i64p(b), threshold=0.9, max_pairs=4, cnt_p=C.byref(cnt)):
        return lib.pcv_searcher_find_duplicates(s, None, 0, threshold, max_pairs, a_p, b_p, None, cnt_p, None)

    def message():
        msg = lib.pcv_last_error().decode()
        assert "find_duplicates" in msg
        return msg

    assert call(None) == PCV_ERR_INVALID
    assert "searcher is NULL" in message()
    assert call(fake, a_p=None) == PCV_ERR_INVALID
    assert "is NULL" in message()
    assert call(fake, b_p=None) == PCV_ERR_INVALID
    assert "is NULL" in message()
    assert call(fake, cnt_p=None) == PCV_ERR_INVALID
    assert "is NULL" in message()
    for m in (0, -1, PCV_MAX_DUPLICATE_PAIRS + 1, 1 << 40):
        assert call(fake, max_pairs=m) == PCV_ERR_INVALID
        assert "max_pairs %d outside [1,%d]" % (m, PCV_MAX_DUPLICATE_PAIRS) in message()
    assert call(fake, threshold=float("nan")) == PCV_ERR_INVALID
    assert "threshold is NaN" in message()
    for t in (-1.0, -2.5, float(np.nextafter(np.float32(1.0), np.float32(2.0))), 3.0, float("inf"), float("-inf")):
        assert call(fake, threshold=t) == PCV_ERR_INVALID
        assert "threshold" in message() and "outside (-1, 1]" in message()
    assert cnt.value == -5  # nothing was written
    st = _ffi.DuplicateStats()
    assert lib.pcv_searcher_last_duplicate_stats(None, C.byref(st)) == PCV_ERR_INVALID
    assert lib.pcv_searcher_last_duplicate_stats(fake, None) == PCV_ERR_INVALID


def union_find_groups(a, b):
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            x = parent[x]
        return x

    for x, y in zip(a, b):
        rx, ry = find(int(x)), find(int(y))
        parent[max(rx, ry)] = min(rx, ry)
    ids = sorted(parent)
    return np.array(ids, dtype=np.int64), np.array([find(i) for i in ids], dtype=np.int64)


GROUP_CASES = {
    "none": ([], [], [], []),
    "chain": ([5, 3, 9], [3, 9, 1], [1, 3, 5, 9], [1, 1, 1, 1]),
    "two_components": ([10, 40, 20], [20, 50, 30], [10, 20, 30, 40, 50], [10, 10, 10, 40, 40]),
    "self_pair": ([7], [7], [7], [7]),
    "repeated": ([2, 2, 8, 2], [8, 8, 2, 8], [2, 8], [2, 2]),
    "negative": ([-4, 6, -9], [6, -9, 11], [-9, -4, 6, 11], [-9, -9, -9, -9]),
}


@pytest.mark.parametrize("case", sorted(GROUP_CASES))
def test_duplicate_groups(case):
    a, b, want_ids, want_group = GROUP_CASES[case]
    ids, group = pa.duplicate_groups(a, b)
    assert ids.dtype == np.int64 and group.dtype == np.int64
    assert ids.tolist() == want_ids and group.tolist() == want_group


def test_duplicate_groups_capacity_too_small():
    lib = _ffi.lib()
    a = np.array([5, 3, 9], dtype=np.int64)
    b = np.array([3, 9, 1], dtype=np.int64)
    ids = np.full(4, -77, dtype=np.int64)
    group = np.full(4, -77, dtype=np.int64)
    n = C.c_int64(-1)
    assert lib.pcv_duplicate_groups(_ffi.i64p(a), _ffi.i64p(b), 3, _ffi.i64p(ids), _ffi.i64p(group), 3, C.byref(n)) == PCV_ERR_INVALID
    assert n.value == 4 and (ids == -77).all() and (group == -77).all()
    assert lib.pcv_duplicate_groups(_ffi.i64p(a), _ffi.i64p(b), 3, _ffi.i64p(ids), _ffi.i64p(group), 4, C.byref(n)) == 0
    assert n.value == 4 and ids.tolist() == [1, 3, 5, 9] and group.tolist() == [1, 1, 1, 1]
    assert lib.pcv_duplicate_groups(_ffi.i64p(a), _ffi.i64p(b), 3, _ffi.i64p(ids), _ffi.i64p(group), 4, None) == PCV_ERR_INVALID
    assert lib.pcv_duplicate_groups(None, _ffi.i64p(b), 3, _ffi.i64p(ids), _ffi.i64p(group), 4, C.byref(n)) == PCV_ERR_INVALID
    assert lib.pcv_duplicate_groups(_ffi.i64p(a), _ffi.i64p(b), -1, _ffi.i64p(ids), _ffi.i64p(group), 4, C.byref(n)) == PCV_ERR_INVALID


def test_duplicate_groups_against_union_find():
    rng = np.random.default_rng(5)
    pool = np.unique(rng.integers(-10**12, 10**12, size=600))[:500]
    assert pool.size == 500
    pool = pool[rng.permutation(500)]
    a = pool[rng.integers(0, 500, size=2000)]
    b = pool[rng.integers(0, 500, size=2000)]
    ids, group = pa.duplicate_groups(a, b)
    want_ids, want_group = union_find_groups(a, b)
    assert np.array_equal(ids, want_ids) and np.array_equal(group, want_group)
    # sparse pairs: many components
    ids, group = pa.duplicate_groups(a[:150], b[:150])
    want_ids, want_group = union_find_groups(a[:150], b[:150])
    assert np.array_equal(ids, want_ids) and np.array_equal(group, want_group)
    assert len(set(group.tolist())) > 10


def test_python_surface():
    for cls in (pa.Searcher, pa.SearcherView):
        for name in ("find_duplicates", "last_duplicate_stats"):
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("find_duplicates", "last_duplicate_stats"):
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited
    assert callable(pa.duplicate_groups)


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn find_duplicates\(&self,\s*sources: &\[i64\],\s*threshold: f32,\s*max_pairs: usize\) -> \(Vec<\(i64, i64, f32\)>, i64\)"
                  r"(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::find_duplicates"
    assert "ffi::pcv_searcher_find_duplicates(" in m.group(1) and "ffi::PCV_MAX_DUPLICATE_PAIRS" in m.group(1)
    assert search_rs.index("pub fn find_duplicates(") < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_duplicates_program_compiles():
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count(" find_duplicates(") == 2 and "pcv_searcher_find_duplicates(" in hpp  # Searcher and SearcherView
    src = os.path.join(ROOT, "tests", "cpp", "duplicates_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "duplicates_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)
