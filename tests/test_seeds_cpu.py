"""CPU: seed items (pcv_searcher_seeds, pcv_searcher_last_seed_stats, pcv_seed_draw) are declared, exported, bound and present in
the regenerated Rust ffi; the argument checks and the draw need no GPU; the Python, C++ and Rust surfaces reach the call; the
reference the GPU tests compare with (seeds_ref.py) agrees with the definition itself; and a row's weight against itself is 0."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import perceive_amd as pa
from perceive_amd import _ffi
from seeds_ref import METHODS, Reference, bits, brute_force, seed_draw, takes_part, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
PCV_MAX_SEEDS = 4096
ARITY = {"pcv_searcher_seeds": 12, "pcv_searcher_last_seed_stats": 2, "pcv_seed_draw": 4}
STATS = [("rows", "int64_t"), ("participating", "int64_t"), ("steps", "int32_t"), ("method", "int32_t"), ("prep_ms", "float"), ("steps_ms", "float")]


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
    assert re.search(r"enum\s*\{\s*PCV_SEED_FARTHEST\s*=\s*0\s*,\s*PCV_SEED_KMEANSPP\s*=\s*1\s*\}", header)
    m = re.search(r"enum\s*\{\s*PCV_MAX_SEEDS\s*=\s*(\d+)\s*\}", header)
    assert m and int(m.group(1)) == PCV_MAX_SEEDS
    from perceive_amd import search

    assert search.PCV_MAX_SEEDS == PCV_MAX_SEEDS and search._SEED_METHODS == {"farthest": 0, "kmeans++": 1}
    m = re.search(r"typedef struct pcv_seed_stats \{(.*?)\} pcv_seed_stats;", header, flags=re.S)
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    assert fields == STATS
    assert [(n, widths[t]) for n, t in fields] == list(_ffi.SeedStats._fields_)
    assert C.sizeof(_ffi.SeedStats) == 32


def test_regenerated_rust_ffi_is_current():
    path = os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")
    ffi_rs = open(path).read()
    assert ("pub fn pcv_searcher_seeds(s: *mut pcv_searcher, source_ids: *const i64, n_sources: c_int, k: c_int, method: c_int, seed: u64, "
            "first_id: *const i64, out_ids: *mut i64, out_positions: *mut i64, out_totals: *mut i64, out_cover: *mut f32, "
            "out_count: *mut i32) -> c_int;") in ffi_rs
    assert "pub fn pcv_searcher_last_seed_stats(s: *mut pcv_searcher, out: *mut pcv_seed_stats) -> c_int;" in ffi_rs
    assert "pub fn pcv_seed_draw(seed: u64, step: c_int, total: u64, out_t: *mut u64) -> c_int;" in ffi_rs
    for line in ("pub const PCV_SEED_FARTHEST: c_int = 0;", "pub const PCV_SEED_KMEANSPP: c_int = 1;", "pub const PCV_MAX_SEEDS: c_int = 4096;"):
        assert line in ffi_rs
    rust = {"int64_t": "i64", "int32_t": "i32", "float": "f32"}
    want = r"pub struct pcv_seed_stats \{\s*" + r"\s*".join(r"pub %s: %s," % (n, rust[t]) for n, t in STATS) + r"\s*\}"
    assert re.search(want, ffi_rs)
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
    ids = np.full(8, -77, dtype=np.int64)
    pos = np.full(8, -77, dtype=np.int64)
    totals = np.full(8, -77, dtype=np.int64)
    cover = np.full(8, -77, dtype=np.float32)
    count = C.c_int32(-5)
    outs = dict(ids_p=_ffi.i64p(ids), pos_p=_ffi.i64p(pos), totals_p=_ffi.i64p(totals), cover_p=_ffi.f32p(cover), count_p=C.byref(count))

    def call(s, k=3, method=1, **kw):
        a = dict(outs, **kw)
        return lib.pcv_searcher_seeds(s, None, 0, k, method, 7, None, a["ids_p"], a["pos_p"], a["totals_p"], a["cover_p"], a["count_p"])

    def message():
        msg = lib.pcv_last_error().decode()
        assert "seeds" in msg
        return msg

    assert call(None) == PCV_ERR_INVALID
    assert "searcher is NULL" in message()
    for name in outs:
        assert call(fake, **{name: None}) == PCV_ERR_INVALID
        assert "an output is NULL" in message()
    for k in (0, -1, PCV_MAX_SEEDS + 1, 1 << 20):
        assert call(fake, k=k) == PCV_ERR_INVALID
        assert "k %d outside [1,%d]" % (k, PCV_MAX_SEEDS) in message()
    for method in (2, -1, 100):
        assert call(fake, method=method) == PCV_ERR_INVALID
        assert "method %d" % method in message()
    assert count.value == -5  # nothing was written
    assert (ids == -77).all() and (pos == -77).all() and (totals == -77).all() and (cover == -77).all()
    st = _ffi.SeedStats()
    assert lib.pcv_searcher_last_seed_stats(None, C.byref(st)) == PCV_ERR_INVALID
    assert lib.pcv_searcher_last_seed_stats(fake, None) == PCV_ERR_INVALID
    assert b"last_seed_stats" in lib.pcv_last_error()
    t = C.c_uint64(99)
    assert lib.pcv_seed_draw(1, 0, 0, C.byref(t)) == PCV_ERR_INVALID
    assert b"seed_draw: total is 0" in lib.pcv_last_error()
    assert lib.pcv_seed_draw(1, -1, 5, C.byref(t)) == PCV_ERR_INVALID
    assert lib.pcv_seed_draw(1, 0, 5, None) == PCV_ERR_INVALID
    assert t.value == 99
    with pytest.raises(pa.PcvError):
        pa.seed_draw(1, 0, 0)


def test_seed_draw_is_the_formula():
    """pcv_seed_draw (the function seed_pick_kernel calls on the device) against the formula in Python ints."""
    rng = np.random.default_rng(7)
    seeds = [0, 1, (1 << 64) - 1, 0x9E3779B97F4A7C15] + [int(x) for x in rng.integers(0, 1 << 63, size=60, dtype=np.uint64)]
    assert len(seeds) == 64
    seen = set()
    for total in (1, 2, 1 << 32, (1 << 32) + 1, 1 << 62, (1 << 63) - 1):
        for seed in seeds:
            for step in range(8):
                t = pa.seed_draw(seed, step, total)
                assert t == seed_draw(seed, step, total), (seed, step, total)
                assert 0 <= t < total
                seen.add((total, t))
    assert len([1 for total, _t in seen if total == 2]) == 2  # (both halves are drawn)
    assert pa.seed_draw(-1, 3, 1 << 40) == seed_draw((1 << 64) - 1, 3, 1 << 40)  # (a Python seed is taken mod 2^64)


def test_python_surface():
    for cls in (pa.Searcher, pa.SearcherView):
        for name in ("seeds", "last_seed_stats"):
            assert callable(getattr(cls, name)), (cls, name)
            assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited
    src = open(os.path.join(ROOT, "perceive_amd", "search.py")).read()
    body = src[src.index("    def seeds("):src.index("    def last_seed_stats(")]
    assert body.count("pcv_searcher_seeds(") == 1 and "PCV_MAX_SEEDS" in body
    km = src[src.index("    def kmeans("):src.index("    def last_assign_stats(")]
    assert "self.seeds(sources, k, init, seed)" in km and "seed=0" in km
    s = pa.Searcher.__new__(pa.Searcher)  # the checks that come before the handle is used
    with pytest.raises(ValueError):
        pa.Searcher.seeds(s, None, 0)
    with pytest.raises(ValueError):
        pa.Searcher.seeds(s, None, PCV_MAX_SEEDS + 1)
    with pytest.raises(ValueError):
        pa.Searcher.seeds(s, None, 3, method="random")


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn seeds\(&self,\s*sources: &\[i64\],\s*k: usize,\s*kmeanspp: bool,\s*seed: u64,\s*first_id: Option<i64>\) -> "
                  r"Vec<\(i64, i64, i64, f32\)>(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::seeds"
    assert m.group(1).count("ffi::pcv_searcher_seeds(") == 1 and "ffi::PCV_MAX_SEEDS" in m.group(1)
    assert "ffi::PCV_SEED_KMEANSPP" in m.group(1) and "ffi::PCV_SEED_FARTHEST" in m.group(1)
    assert search_rs.index("pub fn seeds(") < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_seeds_program_compiles():
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count(" seeds(") == 2 and hpp.count("pcv_searcher_seeds(") == 1  # Searcher and SearcherView, through seeds_handle
    assert hpp.count(" last_seed_stats(") == 2
    src = os.path.join(ROOT, "tests", "cpp", "seeds_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "seeds_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


def hostile_rows(golden_dir):
    g = np.load(os.path.join(golden_dir, "scan_n77_d100.npz"))
    rows = np.array(g["corpus"], dtype=np.float32)
    ids = (np.arange(77) * 3 + 500).astype(np.int64)
    rows[30] = rows[12]                          # identical rows: once one is a seed the other weighs 0
    rows[31] = rows[12] * np.float32(2.0)        # ... and so does a multiple
    rows[20] = 0.0                               # no cosine
    rows[21] = rows[5] * np.float32(2.0 ** -70)  # |x|^2 below 2^-126: no cosine either
    ids[50] = ids[3]                             # an id carried by two rows
    part = np.ones(77, dtype=bool)
    part[[0, 40, 41]] = False                    # hidden, the first row among them
    return rows, ids, part


def test_reference_is_the_definition(oracle, golden_dir):
    rows, ids, part = hostile_rows(golden_dir)
    live = takes_part(rows, part)
    assert not live[[0, 20, 21, 40, 41]].any() and live.sum() == 72
    ref = Reference(oracle, rows, ids, part)
    for method in METHODS:
        for k in (1, 5, 72, 80):
            for seed, first in ((0, None), (12345, None), (3, int(ids[3])), (3, int(ids[12]))):
                want = brute_force(oracle, rows, ids, k, method, seed, first, part)
                got = ref.seeds(k, method, seed, first)
                for g, w in zip(got[:3], want[:3]):
                    np.testing.assert_array_equal(g, w)
                assert np.isnan(got[3][0]) and np.isnan(want[3][0])
                np.testing.assert_array_equal(bits(got[3][1:]), bits(want[3][1:]))
                n = len(got[0])
                assert n <= min(k, 72) and got[2][0] == 72 and (np.diff(got[2][1:]) < 0).all()  # rows, then a potential that only falls
                assert not np.isin(got[1], np.nonzero(~live)[0]).any() and len(set(got[1].tolist())) == n
                if first is not None:
                    assert got[1][0] == (3 if first == ids[3] else 12)  # the first row by position that carries the id
                elif method == "farthest":
                    assert got[1][0] == 1  # the first participating row
                if k >= 72:  # rows 12, 30 and 31 point one way: two of them are never picked, and the picks stop there
                    assert n == 70 and len(set(got[1].tolist()) & {12, 30, 31}) == 1
    for first in (int(ids[0]), int(ids[20]), 7):  # carried by a hidden row only, by a row without a cosine only, by nobody
        with pytest.raises(ValueError):
            ref.seeds(3, "kmeans++", 0, first)
        with pytest.raises(ValueError):
            brute_force(oracle, rows, ids, 3, "kmeans++", 0, first, part)
    none = Reference(oracle, rows, ids, np.zeros(77, dtype=bool)).seeds(4, "farthest")
    assert all(len(x) == 0 for x in none)


@pytest.mark.parametrize("name", ["scan_n77_d100", "scan_n1000_d384"])
def test_a_rows_weight_against_itself_is_zero(oracle, golden_dir, name):
    """What ends the picks and keeps a seed from being drawn twice: c(r, r) is within 2^-51 of 1, and every such value has weight 0."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    rows = np.ascontiguousarray(np.array(g["corpus"], dtype=np.float32))
    live = np.nonzero(takes_part(rows))[0]
    assert live.size >= 77
    c = np.array([oracle.canonical_score(rows[r], rows[r]) for r in live])
    assert (np.abs(c - 1.0) <= 2.0 ** -51).all()
    assert (weights(c) == 0).all()
    assert weights(np.array([1.0 - 2.0 ** -51, 1.0 + 2.0 ** -51, 1.0 - 2.0 ** -34])).tolist() == [0, 0, 0]
    assert weights(np.array([1.0 - 2.0 ** -33, 1.0 - 3 * 2.0 ** -33, 0.0, -1.0, -1.0 - 2.0 ** -52])).tolist() == [0, 2, 1 << 32, 1 << 33, 1 << 33]
