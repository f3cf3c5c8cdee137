"""CPU: boosted search (pcv_searcher_search_boosted) is declared, exported, bound and present in the regenerated Rust ffi; the struct
layout matches the header; the argument checks need no GPU; the Python, C++ and Rust surfaces reach the call; the reference of
tests/boost_ref.py does what the definition says on a list small enough to check by hand and at the extremes of int64; and
recency_boost returns what it promises."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import boost_ref
import grouped_ref
import perceive_amd as pa
from boost_ref import Boost
from perceive_amd import _ffi
from perceive_amd.search import recency_boost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
PCV_MAX_RESULTS = 128
PCV_MAX_BOOST_KNOTS = 16
PCV_MAX_BOOST_POOL = 4096
PCV_NO_VALUE = -(1 << 63)
I64 = np.iinfo(np.int64)
NAME = "pcv_searcher_search_boosted"


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "perceive_hip.h")).read(), flags=re.S)


def test_declared_exported_and_bound():
    header = header_text()
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pcv_[a-z0-9_]+)", out))
    lib = _ffi.lib()
    assert re.search(r"\b%s\s*\(" % NAME, header)
    assert NAME in exported
    assert NAME in _ffi.SYMBOLS and getattr(lib, NAME).argtypes
    assert len(_ffi.SYMBOLS[NAME][1]) == 16
    m = re.search(r"enum\s*\{\s*PCV_MAX_BOOST_KNOTS\s*=\s*(\d+)\s*,\s*PCV_MAX_BOOST_POOL\s*=\s*(\d+)\s*\}", header)
    assert m and (int(m.group(1)), int(m.group(2))) == (PCV_MAX_BOOST_KNOTS, PCV_MAX_BOOST_POOL)
    from perceive_amd import search

    assert (search.PCV_MAX_BOOST_KNOTS, search.PCV_MAX_BOOST_POOL) == (PCV_MAX_BOOST_KNOTS, PCV_MAX_BOOST_POOL)
    assert (pa.PCV_MAX_BOOST_KNOTS, pa.PCV_MAX_BOOST_POOL) == (PCV_MAX_BOOST_KNOTS, PCV_MAX_BOOST_POOL)
    assert pa.recency_boost is search.recency_boost is recency_boost
    assert (boost_ref.NO_VALUE, boost_ref.STEP, boost_ref.MAX_KNOTS, boost_ref.MAX_POOL) == (PCV_NO_VALUE, PCV_MAX_RESULTS, PCV_MAX_BOOST_KNOTS,
                                                                                              PCV_MAX_BOOST_POOL)
    assert boost_ref.default_pool is grouped_ref.default_pool and boost_ref.default_pool(10) == 128 and boost_ref.default_pool(128) == 1024
    # the header says what is not in scope
    text = open(os.path.join(ROOT, "include", "perceive_hip.h")).read()
    doc = text[text.index("/* Boosted results"):text.index("enum { PCV_MAX_BOOST_KNOTS")]
    for phrase in ("Not in scope", "sharded form", "device-resident output", "predicate combined with the boost", "group table", "float"):
        assert phrase in " ".join(doc.replace("*", " ").split()), phrase


def test_struct_layout_matches_the_header():
    header = header_text()
    m = re.search(r"struct pcv_boost \{(.*?)\};\s*typedef struct pcv_boost pcv_boost;", header, flags=re.S)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            ctype, name = decl.split()
            arr = re.match(r"(\w+)\[(\w+)\]$", name)
            fields.append((arr.group(1), ctype, arr.group(2)) if arr else (name, ctype, None))
    assert fields == [("n_knots", "int32_t", None), ("knot_values", "int64_t", "PCV_MAX_BOOST_KNOTS"),
                      ("knot_boosts", "double", "PCV_MAX_BOOST_KNOTS"), ("unset_boost", "double", None)]
    widths = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    want = [(n, widths[t] if a is None else widths[t] * PCV_MAX_BOOST_KNOTS) for n, t, a in fields]
    got = list(_ffi.Boost._fields_)
    assert [n for n, _t in got] == [n for n, _t in want]
    for (_n, gt), (_m, wt) in zip(got, want):
        assert C.sizeof(gt) == C.sizeof(wt) and (getattr(gt, "_length_", None), getattr(gt, "_type_", gt)) == (getattr(wt, "_length_", None), getattr(wt, "_type_", wt))
    # the C layout: 4 bytes and 4 of padding, 16 x 8, 16 x 8, 8
    assert C.sizeof(_ffi.Boost) == 8 + 128 + 128 + 8
    assert (_ffi.Boost.n_knots.offset, _ffi.Boost.knot_values.offset, _ffi.Boost.knot_boosts.offset, _ffi.Boost.unset_boost.offset) == (0, 8, 136, 264)
    # ... and the compiler agrees
    prog = ('#include <stddef.h>\n#include <stdio.h>\n#include "perceive_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(pcv_boost), '
            'offsetof(pcv_boost, n_knots), offsetof(pcv_boost, knot_values), offsetof(pcv_boost, knot_boosts), offsetof(pcv_boost, unset_boost)); return 0; }\n')
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True, capture_output=True, text=True)
        assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["272", "0", "8", "136", "264"]


def test_regenerated_rust_ffi_is_current():
    path = os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")
    ffi_rs = open(path).read()
    for decl in (
        "pub fn pcv_searcher_search_boosted(s: *mut pcv_searcher, queries: *const f32, n_queries: c_int, source_ids: *const i64, "
        "n_sources: c_int, num_results: c_int, pool: c_int, boost: *const pcv_boost, out_ids: *mut i64, out_scores: *mut f32, "
        "out_boosted: *mut f64, out_values: *mut i64, out_ranks: *mut i32, out_counts: *mut i32, out_examined: *mut i32, out_exact: *mut u8) -> c_int;",
        "pub const PCV_MAX_BOOST_KNOTS: c_int = %d;" % PCV_MAX_BOOST_KNOTS,
        "pub const PCV_MAX_BOOST_POOL: c_int = %d;" % PCV_MAX_BOOST_POOL,
    ):
        assert decl in ffi_rs, decl
    m = re.search(r"#\[repr\(C\)\]\n#\[derive\(Debug, Clone, Copy, Default\)\]\npub struct pcv_boost \{\s*pub n_knots: i32,\s*pub knot_values: \[i64; 16\],\s*"
                  r"pub knot_boosts: \[f64; 16\],\s*pub unset_boost: f64,\s*\}", ffi_rs)
    assert m
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


def message():
    msg = _ffi.lib().pcv_last_error().decode()
    assert "search_boosted: " in msg, msg
    return msg[msg.index("search_boosted: "):]


def make_boost(values, boosts, unset=0.0, n=None):
    b = _ffi.Boost()
    b.n_knots = len(values) if n is None else n
    for j, (v, w) in enumerate(zip(values, boosts)):
        b.knot_values[j] = v
        b.knot_boosts[j] = w
    b.unset_boost = unset
    return b


def test_bad_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    fake = C.c_void_p(1)  # never dereferenced: the argument checks come first
    q = np.zeros((2, 8), dtype=np.float32)
    ids = np.zeros((2, 4), dtype=np.int64)
    cnt = np.zeros(2, dtype=np.int32)
    good = make_boost([0, 10], [0.0, 1.0])

    def call(s, q_p, nq, k=4, pool=128, boost=good):
        return lib.pcv_searcher_search_boosted(s, q_p, nq, None, 0, k, pool, C.byref(boost) if boost is not None else None, _ffi.i64p(ids), None, None,
                                               None, None, _ffi.i32p(cnt), None, None)

    assert call(None, _ffi.f32p(q), 2) == PCV_ERR_INVALID
    assert message().startswith("search_boosted: searcher is NULL")
    assert call(fake, None, 2) == PCV_ERR_INVALID
    assert message().startswith("search_boosted: no queries")
    for nq in (0, -3):
        assert call(fake, _ffi.f32p(q), nq) == PCV_ERR_INVALID
        assert message().startswith("search_boosted: no queries")
    for k in (0, -1, PCV_MAX_RESULTS + 1, 1 << 20):
        assert call(fake, _ffi.f32p(q), 2, k=k, pool=PCV_MAX_BOOST_POOL) == PCV_ERR_INVALID
        assert message().startswith("search_boosted: num_results %d outside [1,%d]" % (k, PCV_MAX_RESULTS))
    for k, pool in ((4, 3), (4, 0), (4, -5), (4, PCV_MAX_BOOST_POOL + 1), (128, 127)):
        assert call(fake, _ffi.f32p(q), 2, k=k, pool=pool) == PCV_ERR_INVALID
        assert message().startswith("search_boosted: pool %d outside" % pool)
    assert call(fake, _ffi.f32p(q), 2, boost=None) == PCV_ERR_INVALID
    assert message().startswith("search_boosted: boost is NULL")
    for n in (0, -1, PCV_MAX_BOOST_KNOTS + 1, 1 << 30):
        assert call(fake, _ffi.f32p(q), 2, boost=make_boost([0, 10], [0.0, 1.0], n=n)) == PCV_ERR_INVALID
        assert message().startswith("search_boosted: n_knots %d outside [1,%d]" % (n, PCV_MAX_BOOST_KNOTS))
    for values in ([0, 0], [5, 4], [0, 10, 10], [0, 10, 9, 20], list(range(15)) + [3]):
        assert call(fake, _ffi.f32p(q), 2, boost=make_boost(values, [0.0] * len(values))) == PCV_ERR_INVALID
        assert message().startswith("search_boosted: knot values are not strictly increasing")
    for values in ([PCV_NO_VALUE], [PCV_NO_VALUE, 0]):
        assert call(fake, _ffi.f32p(q), 2, boost=make_boost(values, [0.0] * len(values))) == PCV_ERR_INVALID
        assert message().startswith("search_boosted: knot value 0 is PCV_NO_VALUE")
    for bad in (np.nan, np.inf, -np.inf):
        assert call(fake, _ffi.f32p(q), 2, boost=make_boost([0, 10], [0.0, bad])) == PCV_ERR_INVALID
        assert message().startswith("search_boosted: knot boost 1 is not finite")
        assert call(fake, _ffi.f32p(q), 2, boost=make_boost([0, 10], [0.0, 1.0], unset=bad)) == PCV_ERR_INVALID
        assert message().startswith("search_boosted: unset_boost is not finite")
    # what lies behind the knots in use is not looked at
    odd = make_boost([0, 10, 5, PCV_NO_VALUE], [0.0, 1.0, np.nan, np.inf], n=2)
    assert call(None, _ffi.f32p(q), 2, boost=odd) == PCV_ERR_INVALID
    assert message().startswith("search_boosted: searcher is NULL")


def test_python_surface():
    names = ("search_boosted", "search_boosted_vector", "search_boosted_like_item")
    for name in names:
        assert callable(getattr(pa.Searcher, name))
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited
    b = pa.Searcher._boost([1, 5], [0.25, 0.5], 0.125)
    assert (b.n_knots, list(b.knot_values)[:3], list(b.knot_boosts)[:3], b.unset_boost) == (2, [1, 5, 0], [0.25, 0.5, 0.0], 0.125)
    b = pa.Searcher._boost([I64.min + 1, I64.max], [0.0, 1.0], 0.0)
    assert list(b.knot_values)[:2] == [I64.min + 1, I64.max]
    with pytest.raises(ValueError):
        pa.Searcher._boost([1, 5], [0.25], 0.0)


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn search_vector_boosted\(\s*&self,\s*sources: &\[i64\],\s*num_results: usize,\s*vector: Vec<f32>,\s*knots: &\[\(i64, f64\)\],\s*"
                  r"unset_boost: f64,\s*pool: Option<usize>,?\s*\) -> \(Vec<\(SearchItem, f64, i64\)>, bool\)(.*?)\n    }\n", search_rs, flags=re.S)
    assert m, "Searcher::search_vector_boosted"
    body = m.group(1)
    assert "ffi::pcv_searcher_search_boosted(" in body and "ffi::PCV_MAX_BOOST_POOL" in body and "ffi::PCV_MAX_BOOST_KNOTS" in body
    assert "ffi::pcv_boost::default()" in body and "ffi::PCV_NO_VALUE" in body
    assert search_rs.index("pub fn search_vector_boosted(") < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_boost_program_compiles():
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count("search_vector_boosted(") == 2 and "pcv_searcher_search_boosted(" in hpp  # Searcher and SearcherView
    assert "struct Boost {" in hpp and "struct BoostedItem {" in hpp
    src = os.path.join(ROOT, "tests", "cpp", "boost_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "boost_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


def test_reference_on_a_hand_made_list():
    # eight entries, best first.  Knots (10, 0.0), (20, 0.5), (40, 0.25): a value on a knot, between knots, beyond both ends; entry 3
    # has no value (unset_boost 0.125); entries 0, 2 and 4 tie in m, decided by rank.  Every number is a dyadic fraction: the sums are exact.
    rel = [0.75, 0.5, 0.5, 0.4375, 0.375, 0.25, 0.125, 0.0]
    values = [5, 20, 15, None, 30, 40, 100, 10]
    boost = Boost([10, 20, 40], [0.0, 0.5, 0.25], 0.125)
    b = [float(boost(v)) for v in values]
    #        below   knot  mid    unset  mid    knot   above  knot
    assert b == [0.0, 0.5, 0.25, 0.125, 0.375, 0.25, 0.25, 0.0]
    m = [r + x for r, x in zip(rel, b)]
    assert m == [0.75, 1.0, 0.75, 0.5625, 0.75, 0.5, 0.375, 0.0]
    assert float(boost.b_max) == 0.5
    # the whole list: m descending, the three 0.75 in rank order
    kept, got_m, examined, exact = boost_ref.walk_list(rel, values, boost, 8, 8)
    assert kept == [1, 0, 2, 4, 3, 5, 6, 7] and [float(x) for x in got_m] == m
    # |L| == pool and (b) fails (m_k = 0.0 < rel_last + b_max = 0.5): the flag is 0 ...
    assert (examined, exact) == (8, False)
    # ... and with a larger pool the list ends inside the step: exact
    assert boost_ref.walk_list(rel, values, boost, 8, 9)[2:] == (8, True)
    # k = 3: the tie between ranks 0, 2 and 4 at 0.75 goes to the lower ranks; m_3 = 0.75 >= 0.0 + 0.5 certifies
    assert boost_ref.walk_list(rel, values, boost, 3, 8)[0::2] == ([1, 0, 2], 8) and boost_ref.walk_list(rel, values, boost, 3, 8)[3] is True
    assert boost_ref.walk_list(rel, values, boost, 1, 8)[0] == [1]
    # a pool that cuts the list: only the prefix is ranked, and the certificate looks at its last entry
    kept, _m, examined, exact = boost_ref.walk_list(rel, values, boost, 2, 3)
    assert (kept, examined, exact) == ([1, 0], 3, False)  # m_2 = 0.75 < rel[2] + 0.5 = 1.0
    kept, _m, examined, exact = boost_ref.walk_list(rel, values, boost, 2, 2)
    assert (kept, examined, exact) == ([1, 0], 2, False)
    # a tie between a kept row and a later one with equal m: ranks 5 and 6 under a boost that lifts 6 to 5's m
    tie = Boost([40, 100], [0.0, 0.125], 0.0)
    assert float(rel[5] + tie(values[5])) == float(rel[6] + tie(values[6])) == 0.25
    kept, _m, _e, _x = boost_ref.walk_list(rel, values, tie, 6, 9)
    assert kept == [0, 1, 2, 3, 4, 5]  # 5 before 6
    assert boost_ref.brute_list(rel, values, tie, 7)[0] == [0, 1, 2, 3, 4, 5, 6]
    # the brute force agrees with an exact walk
    assert boost_ref.brute_list(rel, values, boost, 3)[0] == [1, 0, 2]
    # steps of 128: a list of 300 falling relevances, a boost of 1.0 on the entry at rank 200 alone
    rel = [1.0 - r / 1024.0 for r in range(300)]
    values = [7 if r == 200 else None for r in range(300)]
    one = Boost([7], [1.0], 0.0)
    kept, _m, examined, exact = boost_ref.walk_list(rel, values, one, 1, 4096)
    assert (kept, examined, exact) == ([200], 256, True)  # (b) fails after 128 (1.0 < rel[127] + 1) and holds once the row is seen
    late = [7 if r == 299 else None for r in range(300)]
    assert boost_ref.walk_list(rel, late, one, 1, 4096)[0::2] == ([299], 300) and boost_ref.walk_list(rel, late, one, 1, 4096)[3] is True  # (a)
    kept, _m, examined, exact = boost_ref.walk_list(rel, values, one, 1, 129)
    assert (kept, examined, exact) == ([0], 129, False)  # the last step is one entry long
    kept, _m, examined, exact = boost_ref.walk_list(rel, values, one, 1, 256)
    assert (kept, examined, exact) == ([200], 256, True)  # m = 1 + 824/1024 >= rel[255] + 1
    zero = Boost([0], [0.0], 0.0)
    assert boost_ref.walk_list(rel, values, zero, 10, 4096)[0::2] == (list(range(10)), 128)  # one step certifies a zero boost
    # one knot is a constant; a step function is two knots at v and v + 1
    assert [float(Boost([3], [0.5], 0.25)(v)) for v in (I64.min + 1, 3, I64.max, None, PCV_NO_VALUE)] == [0.5, 0.5, 0.5, 0.25, 0.25]
    step = Boost([9, 10], [0.0, 4.0])
    assert [float(step(v)) for v in (-5, 9, 10, 11)] == [0.0, 0.0, 4.0, 4.0]

    # the values follow the ids
    class FakeOracle:
        def topk(self, queries, rows, k, metric=0):
            n = rows.shape[0]
            return np.arange(n)[None, :], np.linspace(0.5, 0.25, n)[None, :], np.array([n])

    ids = np.array([50, 60, 60, 70, 80], dtype=np.int64)
    ref = boost_ref.BoostReference(FakeOracle(), np.zeros((1, 4), np.float32), np.zeros((5, 4), np.float32), ids, "cosine")
    w = ref.walk(0, 2, 128, {60: 100, 80: 200}, Boost([100, 200], [0.25, 1.0]))
    assert w.ids.tolist() == [80, 60] and w.ranks.tolist() == [4, 1] and w.values.tolist() == [200, 100] and (w.examined, w.exact) == (5, True)
    assert w.boosted.tolist() == [1.25, 0.4375 + 0.25]
    np.testing.assert_array_equal(w.scores.view(np.uint32), np.array([0.25, 0.4375], np.float32).view(np.uint32))
    w = ref.walk(0, 3, 128, {}, Boost([0], [1.0], -1.0), allowed=np.array([1, 3, 4]))
    assert w.ids.tolist() == [60, 70, 80] and w.values.tolist() == [PCV_NO_VALUE] * 3 and w.ranks.tolist() == [0, 1, 2]
    d = boost_ref.BoostReference(FakeOracle(), np.zeros((1, 4), np.float32), np.zeros((5, 4), np.float32), ids, "dot")
    assert d.walk(0, 1, 128, {}, Boost([0], [0.0])).boosted.tolist() == [0.125]  # rel = c / dim


def test_boost_at_the_extremes_of_int64():
    lo, hi = I64.min + 1, I64.max
    boost = Boost([lo, hi], [1.0, 3.0])
    # one below the upper knot: the wrapped difference is 2^64 - 3 of 2^64 - 2, both of which round to 2^64 as doubles — t is 1, the
    # sum lands on the knot and the clamp holds it there
    v = hi - 1
    assert (v - lo) % (1 << 64) == (1 << 64) - 3 and (hi - lo) % (1 << 64) == (1 << 64) - 2
    assert float((v - lo) % (1 << 64)) == float((hi - lo) % (1 << 64)) == 2.0 ** 64
    assert float(boost(v)) == 3.0
    # the middle and the ends
    assert float(boost(0)) == 2.0 and float(boost(lo)) == 1.0 and float(boost(hi)) == 3.0 and float(boost(lo + 1)) == 1.0 + 2.0 ** -63
    assert float(boost(-1)) == 2.0 and float(boost(1 << 62)) == 2.5
    # a falling segment: the clamp is into [min, max] of the two boosts
    down = Boost([lo, hi], [3.0, 1.0])
    assert float(down(v)) == 1.0 and float(down(0)) == 2.0
    # the sum can land an ulp past the knot without the clamp: scan for it on a short segment
    worst = 0
    for a, b in ((0.1, 0.7), (-0.3, 0.9), (1e-3, 1.1e-3), (0.7, 0.1)):
        seg = Boost([0, 1000], [a, b])
        for x in range(1001):
            got = float(seg(x))
            assert min(a, b) <= got <= max(a, b)
            t = np.float64(float(x)) / np.float64(1000.0)
            raw = float(np.float64(a) + t * (np.float64(b) - np.float64(a)))
            worst += raw < min(a, b) or raw > max(a, b)
    print("unclamped values past a knot:", worst)
    # a difference that does not fit int64 but fits uint64
    wide = Boost([-(1 << 62) - 5, (1 << 62) + 5], [0.0, 1.0])
    assert float(wide(0)) == 0.5
    assert float(wide.b_max) == 1.0 and float(Boost([0], [-2.0], -1.0).b_max) == -1.0


def test_recency_boost():
    now, half = 1_700_000_000, 86_400 * 7
    for knots in (1, 2, 5, PCV_MAX_BOOST_KNOTS):
        values, boosts = pa.recency_boost(now, half, 0.25, knots)
        assert len(values) == len(boosts) == knots
        assert all(isinstance(v, int) for v in values) and all(a < b for a, b in zip(values, values[1:]))
        assert values[-1] == now and boosts[-1] == 0.25
        assert all(0.0 <= b <= 0.25 for b in boosts) and all(a < b for a, b in zip(boosts, boosts[1:]))
        for v, b in zip(values, boosts):
            assert abs(b - 0.25 * 2.0 ** (-(now - v) / half)) <= 1e-15
        Boost(values, boosts)  # (what the call would accept)
    values, boosts = pa.recency_boost(now, half, 0.25)
    assert len(values) == PCV_MAX_BOOST_KNOTS and now - values[0] == round(half * (2.0 ** 5 - 1.0))
    gaps = [b - a for a, b in zip(values, values[1:])]
    assert all(a > b for a, b in zip(gaps, gaps[1:]))  # geometric going back: the newest gaps are the shortest
    assert pa.recency_boost(now, half, 0.25) == (values, boosts)  # a plain function of its arguments
    tiny = pa.recency_boost(100, 1, 1.0, 8)[0]  # a half-life so short that rounding would repeat an age
    assert all(a < b for a, b in zip(tiny, tiny[1:])) and tiny[-1] == 100
    assert pa.recency_boost(now, half, 0.0, 3)[1] == [0.0, 0.0, 0.0]
    for bad in (lambda: pa.recency_boost(now, 0, 1.0), lambda: pa.recency_boost(now, half, 1.0, 0), lambda: pa.recency_boost(now, half, 1.0, 17),
                lambda: pa.recency_boost(I64.min + 10, half, 1.0)):
        with pytest.raises(ValueError):
            bad()
