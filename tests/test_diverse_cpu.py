"""CPU: diverse results (pcv_searcher_search_diverse) are declared, exported, bound and present in the regenerated Rust ffi; the
argument checks need no GPU; the Python, C++ and Rust surfaces reach the call; and the reference the GPU tests compare with
(tests/diverse_ref.py) has the properties the definition promises."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import diverse_ref as dr
import perceive_amd as pa
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
NAME = "pcv_searcher_search_diverse"
PCV_MAX_RESULTS = 128
PCV_MAX_DIVERSE_POOL = 4096
# the setting of the certificate checks, here and in tests/test_diverse_gpu.py: on the planted cosine corpus (seed 5) the anchor
# queries are certified (their picks stay in the families, far above the pool's last entry) and the Gaussian queries are not
CERT = dict(lam=0.9, k=10, pool=128)


def test_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "perceive_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pcv_[a-z0-9_]+)", out))
    lib = _ffi.lib()
    assert re.search(r"\b%s\s*\(" % NAME, header)
    assert NAME in exported
    assert NAME in _ffi.SYMBOLS and getattr(lib, NAME).argtypes
    assert len(_ffi.SYMBOLS[NAME][1]) == 15
    m = re.search(r"enum\s*\{\s*PCV_MAX_DIVERSE_POOL\s*=\s*(\d+)\s*\}", header)
    assert m and int(m.group(1)) == PCV_MAX_DIVERSE_POOL
    from perceive_amd import search

    assert search.PCV_MAX_DIVERSE_POOL == PCV_MAX_DIVERSE_POOL
    # placed after the grouped-results block
    assert header.index("pcv_searcher_search_grouped(") < header.index(NAME + "(") < header.index("pcv_searcher_find_duplicates(")


def test_regenerated_rust_ffi_is_current():
    ffi_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")).read()
    assert ("pub fn pcv_searcher_search_diverse(s: *mut pcv_searcher, queries: *const f32, n_queries: c_int, source_ids: *const i64, "
            "n_sources: c_int, num_results: c_int, lambda: f32, pool: c_int, out_ids: *mut i64, out_scores: *mut f32, "
            "out_marginal: *mut f64, out_ranks: *mut i32, out_counts: *mut i32, out_examined: *mut i32, out_exact: *mut u8) -> c_int;") in ffi_rs
    assert "pub const PCV_MAX_DIVERSE_POOL: c_int = %d;" % PCV_MAX_DIVERSE_POOL in ffi_rs
    # (that the file is what the generator writes from the header today: tests/test_distinct_cpu.py)


def test_bad_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    fake = C.c_void_p(1)  # never dereferenced: the argument checks come first
    q = np.zeros((2, 8), dtype=np.float32)
    ids = np.zeros((2, 4), dtype=np.int64)
    cnt = np.zeros(2, dtype=np.int32)

    def call(s, q_p, nq, k=4, lam=0.5, pool=128):
        return lib.pcv_searcher_search_diverse(s, q_p, nq, None, 0, k, lam, pool, _ffi.i64p(ids), None, None, None, _ffi.i32p(cnt), None, None)

    def message():
        msg = lib.pcv_last_error().decode()
        assert "search_diverse" in msg
        return msg

    assert call(None, _ffi.f32p(q), 2) == PCV_ERR_INVALID
    assert "searcher is NULL" in message()
    assert call(fake, None, 2) == PCV_ERR_INVALID
    assert "no queries" in message()
    for nq in (0, -3):
        assert call(fake, _ffi.f32p(q), nq) == PCV_ERR_INVALID
        assert "no queries" in message()
    for k in (0, -1, PCV_MAX_RESULTS + 1, 1 << 20):
        assert call(fake, _ffi.f32p(q), 2, k=k, pool=PCV_MAX_DIVERSE_POOL) == PCV_ERR_INVALID
        assert "num_results %d outside [1,%d]" % (k, PCV_MAX_RESULTS) in message()
    for k, pool in ((4, 3), (4, 0), (4, -5), (4, PCV_MAX_DIVERSE_POOL + 1), (128, 127)):
        assert call(fake, _ffi.f32p(q), 2, k=k, pool=pool) == PCV_ERR_INVALID
        assert "pool %d outside" % pool in message()
    assert call(fake, _ffi.f32p(q), 2, lam=float("nan")) == PCV_ERR_INVALID
    assert "lambda is NaN" in message()
    for lam in (float(np.nextafter(np.float32(0.0), np.float32(-1.0))), -0.5, float(np.nextafter(np.float32(1.0), np.float32(2.0))), 3.0,
                float("inf"), float("-inf")):
        assert call(fake, _ffi.f32p(q), 2, lam=lam) == PCV_ERR_INVALID
        assert "lambda" in message() and "outside [0, 1]" in message()


def test_python_surface():
    names = ("search_diverse", "search_diverse_vector", "search_diverse_like_item")
    for cls in (pa.Searcher, pa.SearcherView):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    for name in names:
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn search_vector_diverse\(\s*&self,\s*sources: &\[i64\],\s*num_results: usize,\s*vector: Vec<f32>,\s*lambda: f32,\s*"
                  r"pool: Option<usize>,?\s*\) -> Vec<\(SearchItem, f64, i32\)>(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::search_vector_diverse"
    assert "ffi::pcv_searcher_search_diverse(" in m.group(1) and "ffi::PCV_MAX_DIVERSE_POOL" in m.group(1)
    assert search_rs.index("pub fn search_vector_diverse(") < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_diverse_program_compiles():
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count("search_vector_diverse(") == 2 and "pcv_searcher_search_diverse(" in hpp  # Searcher and SearcherView
    src = os.path.join(ROOT, "tests", "cpp", "diverse_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "diverse_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


# ---- the reference itself ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(oracle):
    rows, ids, anchors = dr.planted_corpus("cosine")
    queries = dr.planted_queries("cosine", anchors, rows.shape[1])
    return rows, ids, queries, dr.Reference(oracle, queries, rows, ids, "cosine")


def outside_never_reaches(ref, q, w, pool):
    """the certificate's argument, row by row: whatever was picked before, a row outside the pool has m <= the bound"""
    L, sc = ref.ranked(q)
    worst = -np.inf
    for row, c in zip(L[pool:], sc[pool:]):
        assert ref.rel(c) <= w.rel_last
        lowest = min([ref.cos(row, p) for p in w.rows] + [0.0])  # div is 0 before the first pick, a cosine after it
        assert lowest >= -dr.D0
        a = w.lam * ref.rel(c)
        b = w.mu * lowest
        m = a - b
        assert m <= w.bound, (q, row, m, w.bound)
        worst = max(worst, m)
    return worst


def test_reference_lambda_one_is_the_ranked_list_and_the_first_pick_is_its_head(planted):
    _rows, ids, _queries, ref = planted
    for q in (0, 3, 9, 15):
        for k, pool in ((1, 128), (10, 128), (128, 1024)):
            w = ref.walk(q, k, 1.0, pool)
            np.testing.assert_array_equal(w.ranks, np.arange(k))
            np.testing.assert_array_equal(w.ids, ids[ref.pos[q, :k]])
            np.testing.assert_array_equal(dr.bits64(w.marginal), dr.bits64(ref.sc[q, :k]))  # 1 * rel - 0 * div
        for lam in (0.0, 0.3, 0.5, 0.7, 0.9, 1.0):
            w = ref.walk(q, 10, lam, 128)
            assert w.ranks[0] == 0 and len(set(w.ranks.tolist())) == 10 and w.examined == 128
            assert w.marginal[0] == w.lam * ref.sc[q, 0]


def test_reference_certificate_on_the_planted_corpus(planted):
    _rows, _ids, _queries, ref = planted
    flags = []
    for q in range(16):
        w = ref.walk(q, CERT["k"], CERT["lam"], CERT["pool"])
        full = ref.walk(q, CERT["k"], CERT["lam"], None)
        worst = outside_never_reaches(ref, q, w, CERT["pool"])
        print("query %d: exact %d, smallest pick %.6f, bound %.6f, best outside row %.6f, last rank %d (all of L: %d)" % (
            q, w.exact, w.marginal.min(), w.bound, worst, w.ranks.max(), full.ranks.max()))
        assert full.exact and full.examined == int(ref.cnt[q])
        if w.exact:  # a 1 is a proof
            np.testing.assert_array_equal(w.ranks, full.ranks)
            np.testing.assert_array_equal(dr.bits64(w.marginal), dr.bits64(full.marginal))
        flags.append(w.exact)
    assert flags[:8] == [True] * 8 and flags[8:] == [False] * 8  # both values occur: the anchors are certified, the others not


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_reference_certificate_with_an_antiparallel_pair(oracle, metric):
    """x and -x: the canonical cosine may round past -1 by a few ulps and never past -(1 + 2^-40); at a small lambda the walk wants
    exactly such rows, and the bound still covers every row outside the pool"""
    rng = np.random.default_rng(41)
    N, dim, pool = 400, 96, 32
    rows = rng.standard_normal((N, dim)).astype(np.float32)
    rows[200:260] = -rows[100:160] * rng.uniform(0.5, 2.0, size=(60, 1)).astype(np.float32)
    queries = (rows[100:104] + 0.3 * rng.standard_normal((4, dim))).astype(np.float32)
    ref = dr.Reference(oracle, queries, rows, np.arange(N, dtype=np.int64), metric)
    lowest = min(oracle.lib.orc_canonical_score(ref.ptr[100 + i], ref.ptr[200 + i], dim, 0) for i in range(60))
    assert -dr.D0 <= lowest <= -1.0 + 1e-6
    assert lowest >= -dr.D0 and min(ref.cos(100 + i, 200 + i) for i in range(60)) == lowest
    for lam in (0.05, 0.5, 0.9):
        for q in range(4):
            w = ref.walk(q, 8, lam, pool)
            outside_never_reaches(ref, q, w, pool)
            if w.exact:
                np.testing.assert_array_equal(w.ranks, ref.walk(q, 8, lam, None).ranks)
