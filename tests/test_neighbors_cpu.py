"""CPU: item neighbours (pcv_searcher_neighbors, pcv_searcher_last_neighbor_stats) are declared, exported, bound and present in
the regenerated Rust ffi; the argument checks need no GPU; the Python, C++ and Rust surfaces reach the call; and the reference the
GPU tests compare with (neighbors_ref.py) agrees with the definition itself."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import perceive_amd as pa
from neighbors_ref import bits, brute_force, reference, takes_part
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
PCV_MAX_NEIGHBORS = 64
ARITY = {"pcv_searcher_neighbors": 10, "pcv_searcher_last_neighbor_stats": 2}
STATS = ["rows", "candidates", "listed", "k", "tile_rows", "sample_stride", "spans", "reruns", "prep_ms", "bound_ms", "screen_ms", "rescore_ms",
         "select_ms"]


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
    m = re.search(r"enum\s*\{\s*PCV_MAX_NEIGHBORS\s*=\s*(\d+)\s*\}", header)
    assert m and int(m.group(1)) == PCV_MAX_NEIGHBORS
    from perceive_amd import search

    assert search.PCV_MAX_NEIGHBORS == PCV_MAX_NEIGHBORS
    # the stats struct: the header's fields, in order, with the binding's widths
    m = re.search(r"typedef struct pcv_neighbor_stats \{(.*?)\} pcv_neighbor_stats;", header, flags=re.S)
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, widths[t]) for n, t in fields] == list(_ffi.NeighborStats._fields_)
    assert [n for n, _ in fields] == STATS
    assert [t for _, t in fields] == ["int64_t"] * 3 + ["int32_t"] * 5 + ["float"] * 5
    assert C.sizeof(_ffi.NeighborStats) == 64


def test_regenerated_rust_ffi_is_current():
    path = os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")
    ffi_rs = open(path).read()
    assert ("pub fn pcv_searcher_neighbors(s: *mut pcv_searcher, source_ids: *const i64, n_sources: c_int, k: c_int, capacity: i64, "
            "out_ids: *mut i64, out_neighbor_ids: *mut i64, out_scores: *mut f32, out_counts: *mut i32, out_rows: *mut i64) -> c_int;") in ffi_rs
    assert "pub fn pcv_searcher_last_neighbor_stats(s: *mut pcv_searcher, out: *mut pcv_neighbor_stats) -> c_int;" in ffi_rs
    assert "pub const PCV_MAX_NEIGHBORS: c_int = %d;" % PCV_MAX_NEIGHBORS in ffi_rs
    want = r"pub struct pcv_neighbor_stats \{\s*" + r"\s*".join(
        r"pub %s: %s," % (n, "i64" if i < 3 else "i32" if i < 8 else "f32") for i, n in enumerate(STATS)) + r"\s*\}"
    assert re.search(want, ffi_rs)
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
    ids = np.full(4, -77, dtype=np.int64)
    nbr = np.full((4, 64), -77, dtype=np.int64)
    scores = np.full((4, 64), -77, dtype=np.float32)
    counts = np.full(4, -77, dtype=np.int32)
    rows = C.c_int64(-5)
    arrays = dict(ids_p=_ffi.i64p(ids), nbr_p=_ffi.i64p(nbr), scores_p=_ffi.f32p(scores), counts_p=_ffi.i32p(counts))

    def call(s, k=3, capacity=4, rows_p=C.byref(rows), **kw):
        a = dict(arrays, **kw)
        return lib.pcv_searcher_neighbors(s, None, 0, k, capacity, a["ids_p"], a["nbr_p"], a["scores_p"], a["counts_p"], rows_p)

    def message():
        msg = lib.pcv_last_error().decode()
        assert "neighbors" in msg
        return msg

    assert call(None) == PCV_ERR_INVALID
    assert "searcher is NULL" in message()
    assert call(fake, rows_p=None) == PCV_ERR_INVALID
    assert "out_rows is NULL" in message()
    for k in (0, -1, 65, 1 << 20):
        assert call(fake, k=k) == PCV_ERR_INVALID
        assert "k %d outside [1,%d]" % (k, PCV_MAX_NEIGHBORS) in message()
        assert call(fake, k=k, capacity=0, ids_p=None, nbr_p=None, scores_p=None, counts_p=None) == PCV_ERR_INVALID  # counting only, too
    for cap in (-1, -(1 << 40)):
        assert call(fake, capacity=cap) == PCV_ERR_INVALID
        assert "capacity %d is negative" % cap in message()
    for name in arrays:
        assert call(fake, **{name: None}) == PCV_ERR_INVALID
        assert "is NULL with capacity 4" in message()
        assert call(fake, capacity=0, **{name: None}) == PCV_ERR_INVALID  # counting only means all four NULL
    assert call(None, capacity=0, ids_p=None, nbr_p=None, scores_p=None, counts_p=None) == PCV_ERR_INVALID
    assert "searcher is NULL" in message()
    assert rows.value == -5  # nothing was written
    assert (ids == -77).all() and (nbr == -77).all() and (scores == -77).all() and (counts == -77).all()
    st = _ffi.NeighborStats()
    assert lib.pcv_searcher_last_neighbor_stats(None, C.byref(st)) == PCV_ERR_INVALID
    assert lib.pcv_searcher_last_neighbor_stats(fake, None) == PCV_ERR_INVALID
    assert b"last_neighbor_stats" in lib.pcv_last_error()


def test_python_surface():
    for cls in (pa.Searcher, pa.SearcherView):
        for name in ("neighbors", "last_neighbor_stats"):
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("neighbors", "last_neighbor_stats"):
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited
    src = open(os.path.join(ROOT, "perceive_amd", "search.py")).read()
    body = src[src.index("    def neighbors("):src.index("    def last_neighbor_stats(")]
    assert body.count("pcv_searcher_neighbors(") == 2 and "PCV_MAX_NEIGHBORS" in body  # the count, then the table


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn neighbors\(&self,\s*sources: &\[i64\],\s*k: usize\) -> Vec<\(i64, Vec<\(i64, f32\)>\)>(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::neighbors"
    assert m.group(1).count("ffi::pcv_searcher_neighbors(") == 2 and "ffi::PCV_MAX_NEIGHBORS" in m.group(1)
    assert search_rs.index("pub fn neighbors(") < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_neighbors_program_compiles():
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count(" neighbors(") == 2 and hpp.count("pcv_searcher_neighbors(") == 2  # Searcher and SearcherView; the count, then the table
    assert hpp.count(" last_neighbor_stats(") == 2
    src = os.path.join(ROOT, "tests", "cpp", "neighbors_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "neighbors_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


def test_reference_is_the_definition(oracle, golden_dir):
    g = np.load(os.path.join(golden_dir, "scan_n77_d100.npz"))
    rows = np.array(g["corpus"], dtype=np.float32)
    ids = (np.arange(77) * 3 + 500).astype(np.int64)
    rows[30] = rows[12]                       # a tie: position 12 before position 30 in every list that holds both
    rows[31] = rows[12] * np.float32(2.0)     # ... and 31 behind them: the same cosine bits
    rows[20] = 0.0                            # no cosine
    rows[21] = rows[5] * np.float32(2.0 ** -70)  # |x|^2 below 2^-126: no cosine either
    part = np.ones(77, dtype=bool)
    part[[40, 41]] = False                    # hidden
    live = takes_part(rows, part)
    assert not live[[20, 21, 40, 41]].any() and live.sum() == 73
    for k in (1, 4, 64, 72):
        want = brute_force(oracle, rows, ids, k, part)
        got = reference(oracle, rows, ids, k, part)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[3], want[3])
        used = np.arange(k)[None, :] < want[3][:, None]
        np.testing.assert_array_equal(bits(got[2])[used], bits(want[2])[used])
        assert (got[3][live] == min(k, 72)).all() and (got[3][~live] == 0).all()
        assert not np.isin(got[1], ids[~live]).any()  # a row that takes no part is nobody's neighbour
        if k >= 4:
            assert got[1][12, 0] == ids[30] and got[1][30, 0] == ids[12]
            assert got[1][31, :2].tolist() == [ids[12], ids[30]]
