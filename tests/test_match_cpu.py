"""CPU: item matches (pcv_searcher_match, pcv_searcher_last_match_stats) are declared, exported, bound and present in the regenerated
Rust ffi; the argument checks need no GPU; the Python and C++ surfaces reach the call; and the reference the GPU tests compare with
(match_ref.py) agrees with the definition itself and, on the square, with the neighbours' reference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_ref
import neighbors_ref
import perceive_amd as pa
from duplicates_ref import bits
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
PCV_MAX_NEIGHBORS = 64
ARITY = {"pcv_searcher_match": 13, "pcv_searcher_last_match_stats": 2}
STATS = [("rows", "int64_t"), ("partner_rows", "int64_t"), ("owner_blocks", "int32_t"), ("partner_blocks", "int32_t"), ("candidates", "int64_t"),
         ("listed", "int64_t"), ("k", "int32_t"), ("tile_rows", "int32_t"), ("sample_stride", "int32_t"), ("spans", "int32_t"), ("reruns", "int32_t"),
         ("prep_ms", "float"), ("bound_ms", "float"), ("screen_ms", "float"), ("rescore_ms", "float"), ("select_ms", "float")]


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
    # the stats struct: the header's fields, in order, with the binding's widths
    m = re.search(r"typedef struct pcv_match_stats \{(.*?)\} pcv_match_stats;", header, flags=re.S)
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    assert fields == STATS
    assert [(n, widths[t]) for n, t in fields] == list(_ffi.MatchStats._fields_)
    assert C.sizeof(_ffi.MatchStats) == 80  # no padding: the two int32 block counts fill one 8-byte slot


def test_regenerated_rust_ffi_is_current():
    ffi_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")).read()
    assert ("pub fn pcv_searcher_match(s: *mut pcv_searcher, from_source_ids: *const i64, n_from: c_int, to_source_ids: *const i64, n_to: c_int, "
            "k: c_int, min_score: f32, capacity: i64, out_ids: *mut i64, out_match_ids: *mut i64, out_scores: *mut f32, out_counts: *mut i32, "
            "out_rows: *mut i64) -> c_int;") in ffi_rs
    assert "pub fn pcv_searcher_last_match_stats(s: *mut pcv_searcher, out: *mut pcv_match_stats) -> c_int;" in ffi_rs
    rust = {"int64_t": "i64", "int32_t": "i32", "float": "f32"}
    want = r"pub struct pcv_match_stats \{\s*" + r"\s*".join(r"pub %s: %s," % (n, rust[t]) for n, t in STATS) + r"\s*\}"
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
    mids = np.full((4, 64), -77, dtype=np.int64)
    scores = np.full((4, 64), -77, dtype=np.float32)
    counts = np.full(4, -77, dtype=np.int32)
    rows = C.c_int64(-5)
    arrays = dict(ids_p=_ffi.i64p(ids), mids_p=_ffi.i64p(mids), scores_p=_ffi.f32p(scores), counts_p=_ffi.i32p(counts))
    nothing = dict(capacity=0, ids_p=None, mids_p=None, scores_p=None, counts_p=None)

    def call(s, k=3, min_score=-1.0, capacity=4, rows_p=C.byref(rows), **kw):
        a = dict(arrays, **kw)
        return lib.pcv_searcher_match(s, None, 0, None, 0, k, min_score, capacity, a["ids_p"], a["mids_p"], a["scores_p"], a["counts_p"], rows_p)

    def message():
        msg = lib.pcv_last_error().decode()
        assert "match" in msg
        return msg

    assert call(None) == PCV_ERR_INVALID
    assert "searcher is NULL" in message()
    assert call(fake, rows_p=None) == PCV_ERR_INVALID
    assert "out_rows is NULL" in message()
    for k in (0, -1, 65, 1 << 20):
        assert call(fake, k=k) == PCV_ERR_INVALID
        assert "k %d outside [1,%d]" % (k, PCV_MAX_NEIGHBORS) in message()
        assert call(fake, k=k, **nothing) == PCV_ERR_INVALID  # counting only, too
    assert call(fake, min_score=float("nan")) == PCV_ERR_INVALID
    assert "min_score is NaN" in message()
    for lo in (-1.0000001, 1.0000001, -2.0, 7.0, float("inf"), float("-inf")):
        assert np.float32(lo) < -1 or np.float32(lo) > 1  # (still outside once it is an f32)
        assert call(fake, min_score=lo) == PCV_ERR_INVALID
        assert "outside [-1, 1]" in message()
        assert call(fake, min_score=lo, **nothing) == PCV_ERR_INVALID
    assert call(fake, k=0, min_score=float("nan"), capacity=-1) == PCV_ERR_INVALID  # the order of the checks: k, min_score, capacity
    assert "k 0 outside" in message()
    assert call(fake, min_score=float("nan"), capacity=-1) == PCV_ERR_INVALID
    assert "min_score is NaN" in message()
    for cap in (-1, -(1 << 40)):
        assert call(fake, capacity=cap) == PCV_ERR_INVALID
        assert "capacity %d is negative" % cap in message()
    for name in arrays:
        assert call(fake, **{name: None}) == PCV_ERR_INVALID
        assert "is NULL with capacity 4" in message()
        assert call(fake, capacity=0, **{name: None}) == PCV_ERR_INVALID  # counting only means all four NULL
    assert call(None, **nothing) == PCV_ERR_INVALID
    assert "searcher is NULL" in message()
    assert rows.value == -5  # nothing was written
    assert (ids == -77).all() and (mids == -77).all() and (scores == -77).all() and (counts == -77).all()
    st = _ffi.MatchStats()
    assert lib.pcv_searcher_last_match_stats(None, C.byref(st)) == PCV_ERR_INVALID
    assert lib.pcv_searcher_last_match_stats(fake, None) == PCV_ERR_INVALID
    assert b"last_match_stats" in lib.pcv_last_error()


def test_python_surface():
    for cls in (pa.Searcher, pa.SearcherView):
        for name in ("match", "last_match_stats"):
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("match", "last_match_stats"):
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited
    src = open(os.path.join(ROOT, "perceive_amd", "search.py")).read()
    body = src[src.index("    def match("):src.index("    def last_match_stats(")]
    assert body.count("pcv_searcher_match(") == 2 and "PCV_MAX_NEIGHBORS" in body  # the count, then the table
    # the mirror only converts arguments: no arithmetic on rows or scores, no other call of the library
    assert body.count("_ffi.lib().") == 2 and body.count("_source_filter(") == 2
    for word in ("neighbors(", "search(", "np.sort", "argsort", "np.where", " for ", " while "):
        assert word not in body.split('"""')[2], word


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn matches\(&self,\s*from: &\[i64\],\s*to: &\[i64\],\s*k: usize,\s*min_score: f32\) -> Vec<\(i64, Vec<\(i64, f32\)>\)>(.*?)\n    }\n",
                  search_rs, flags=re.S)
    assert m, "Searcher::matches"
    assert m.group(1).count("ffi::pcv_searcher_match(") == 2 and "ffi::PCV_MAX_NEIGHBORS" in m.group(1)
    assert search_rs.index("pub fn matches(") < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_match_program_compiles():
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count(" match(") == 2 and hpp.count("pcv_searcher_match(") == 2  # Searcher and SearcherView; the count, then the table
    assert hpp.count(" last_match_stats(") == 2 and hpp.count("pcv_searcher_last_match_stats(") == 2
    src = os.path.join(ROOT, "tests", "cpp", "match_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "match_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def small_corpus(golden_dir):
    """about 60 rows in three sources a, b, c (positions 0..19, 20..44, 45..59) with ties, rows without a cosine and hidden rows"""
    g = np.load(os.path.join(golden_dir, "scan_n77_d100.npz"))
    rows = np.array(g["corpus"], dtype=np.float32)[:60]
    ids = (np.arange(60) * 3 + 500).astype(np.int64)
    rows[30] = rows[12]                       # a tie across sources: position 12 before position 30 wherever both are partners
    rows[50] = rows[12] * np.float32(2.0)     # ... and 50 behind them: the same cosine bits
    rows[7] = 0.0                             # no cosine
    rows[47] = rows[5] * np.float32(2.0 ** -70)  # |x|^2 below 2^-126: no cosine either
    ids[33] = ids[3]                          # an item id stored in two sources
    part = np.ones(60, dtype=bool)
    part[[25, 55]] = False                    # hidden
    src = np.repeat([0, 1, 2], [20, 25, 15])
    return np.ascontiguousarray(rows), ids, part, src


SELECTIONS = {
    "disjoint": ([0], [1, 2]),
    "overlapping": ([0, 1], [1, 2]),
    "identical": ([1], [1]),
    "from before to": ([0], [2]),
    "from after to": ([2], [0]),
}


@pytest.mark.parametrize("case", sorted(SELECTIONS))
def test_reference_is_the_definition(oracle, golden_dir, case):
    rows, ids, part, src = small_corpus(golden_dir)
    live = neighbors_ref.takes_part(rows, part)
    assert not live[[7, 47, 25, 55]].any() and live.sum() == 56
    frm, to = SELECTIONS[case]
    owner, partner = np.isin(src, frm), np.isin(src, to)
    assert {"disjoint": not (owner & partner).any(), "overlapping": (owner & partner).any() and (owner ^ partner).any(),
            "identical": (owner == partner).all(), "from before to": np.nonzero(owner)[0].max() < np.nonzero(partner)[0].min(),
            "from after to": np.nonzero(owner)[0].min() > np.nonzero(partner)[0].max()}[case]
    for k in (1, 4, 64):
        for lo in (-1.0, 0.05, 0.999):
            want = match_ref.brute_force(oracle, rows, ids, owner, partner, k, lo, part)
            got = match_ref.reference(oracle, rows, ids, owner, partner, k, lo, part)
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[0], ids[owner])
            np.testing.assert_array_equal(got[3], want[3])
            np.testing.assert_array_equal(got[1], want[1])
            used = np.arange(k)[None, :] < want[3][:, None]
            np.testing.assert_array_equal(bits(got[2])[used], bits(want[2])[used])
            assert np.isnan(got[2][~used]).all() and (got[1][~used] == -1).all()
            assert (got[3][~live[owner]] == 0).all()
            assert not np.isin(got[1], np.setdiff1d(ids[~(live & partner)], ids[live & partner])).any()  # only participating partners
            if lo == -1.0:  # no bound: min(k, partners - [the owner is one])
                P = int((partner & live).sum())
                np.testing.assert_array_equal(got[3][live[owner]], np.minimum(k, P - (partner & live)[owner][live[owner]]))
            else:
                assert (got[2][used].astype(np.float64) >= float(np.float32(lo)) - 1e-7).all() and got[3].sum() < want[3].size * min(k, 40)
    got = match_ref.reference(oracle, rows, ids, owner, partner, 4, -1.0, part)
    if case == "overlapping":  # the tie: 12 is an owner only, 30 both, 50 a partner only; outputs are positions 0..44
        assert got[1][12, :2].tolist() == [ids[30], ids[50]] and got[1][30, 0] == ids[50]
    if case == "from after to":  # outputs are positions 45..59
        assert got[1][50 - 45, 0] == ids[12]


def test_square_reference_is_the_neighbours(oracle, golden_dir):
    rows, ids, part, _src = small_corpus(golden_dir)
    full = np.ones(60, dtype=bool)
    for k in (1, 4, 64):
        got = match_ref.reference(oracle, rows, ids, full, full, k, -1.0, part)
        want = neighbors_ref.reference(oracle, rows, ids, k, part)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(bits(g) if g.dtype == np.float32 else g, bits(w) if w.dtype == np.float32 else w)
