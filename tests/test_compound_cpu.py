"""CPU: compound queries (pcv_searcher_search_compound / _search_compound_like) are declared, exported, bound and present in the
regenerated Rust ffi; the argument checks that can be made before the searcher is looked at need no GPU (the two that need its
dimension — a value that is not finite, a vector without a cosine — are in test_compound_gpu.py); the Python layer packs the offsets
as the header says; the C++ and Rust surfaces reach the calls; the reference of tests/compound_ref.py does what the definition says
on lists small enough to check by hand — a tie at the bound does not certify —; and the inputs test_compound_gpu.py uses reach every
branch of the walk, in the model alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import compound_ref as cr
import perceive_amd as pa
from compound_ref import ALL, ANY, F64
from perceive_amd import _ffi, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
PCV_MAX_RESULTS = 128
NAMES = ("pcv_searcher_search_compound", "pcv_searcher_search_compound_like")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "perceive_hip.h")).read(), flags=re.S)


def test_declared_exported_and_bound():
    header = header_text()
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    lib = _ffi.lib()
    for name, n_args in zip(NAMES, (19, 24)):
        m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, header, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args
        assert name in exported
        assert name in _ffi.SYMBOLS and getattr(lib, name).argtypes and len(_ffi.SYMBOLS[name][1]) == n_args
        # scalar arguments only: no struct goes through either call
        assert "struct" not in m.group(1) and not re.search(r"pcv_\w+\s*\*", m.group(1).replace("pcv_searcher*", ""))
    assert not [s for s in exported if "compound" in s and s not in NAMES and not s.startswith("_Z")]
    # the diagnostic that times the select steps (tools/bench_compound.py)
    timing = "pcv_searcher_last_select_stats"
    assert re.search(r"\b%s\s*\(" % timing, header) and timing in exported and len(_ffi.SYMBOLS[timing][1]) == 3
    assert callable(pa.Searcher.last_select_stats) and lib.pcv_searcher_last_select_stats(None, None, None) == PCV_ERR_INVALID
    m = re.search(r"enum\s*\{\s*PCV_MAX_COMPOUND_PARTS\s*=\s*(\d+)\s*,\s*PCV_MAX_COMPOUND_POOL\s*=\s*(\d+)\s*\}", header)
    assert m and (int(m.group(1)), int(m.group(2))) == (8, 4096)
    m = re.search(r"enum\s*\{\s*PCV_COMPOUND_ALL\s*=\s*(\d+)\s*,\s*PCV_COMPOUND_ANY\s*=\s*(\d+)\s*\}", header)
    assert m and (int(m.group(1)), int(m.group(2))) == (ALL, ANY) == (0, 1)
    assert (search.PCV_MAX_COMPOUND_PARTS, search.PCV_MAX_COMPOUND_POOL, search.COMPOUND_MODES) == (8, 4096, {"all": 0, "any": 1})
    assert (pa.PCV_MAX_COMPOUND_PARTS, pa.PCV_MAX_COMPOUND_POOL) == (8, 4096)
    assert (cr.STEP, cr.MAX_PARTS, cr.MAX_POOL) == (PCV_MAX_RESULTS, 8, 4096)
    assert cr.default_pool(10) == 128 and cr.default_pool(128) == 1024
    text = open(os.path.join(ROOT, "include", "perceive_hip.h")).read()
    doc = " ".join(text[text.index("/* Compound queries"):text.index("enum { PCV_MAX_COMPOUND_PARTS")].replace("*", " ").split())
    for phrase in ("Not in scope", "sharded form", "device-resident output", "weighted-sum mode", "group table", "STRICT"):
        assert phrase in doc, phrase


def test_regenerated_rust_ffi_is_current():
    path = os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")
    ffi_rs = open(path).read()
    for decl in (
        "pub fn pcv_searcher_search_compound(s: *mut pcv_searcher, source_ids: *const i64, n_sources: c_int, num_results: c_int, pool: c_int, "
        "mode: c_int, avoid_weight: f32, want: *const f32, want_offsets: *const i64, avoid: *const f32, avoid_offsets: *const i64, "
        "n_compounds: c_int, out_ids: *mut i64, out_combined: *mut f64, out_part_scores: *mut f32, out_penalties: *mut f64, "
        "out_counts: *mut i32, out_examined: *mut i32, out_exact: *mut u8) -> c_int;",
        "pub fn pcv_searcher_search_compound_like(s: *mut pcv_searcher, source_ids: *const i64,",
        "pub const PCV_MAX_COMPOUND_PARTS: c_int = 8;",
        "pub const PCV_MAX_COMPOUND_POOL: c_int = 4096;",
        "pub const PCV_COMPOUND_ALL: c_int = 0;",
        "pub const PCV_COMPOUND_ANY: c_int = 1;",
    ):
        assert decl in ffi_rs, decl
    import importlib.util
    import tempfile

    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with tempfile.TemporaryDirectory() as tmp:
        gen.OUT = os.path.join(tmp, "ffi.rs")
        gen.main()
        assert open(gen.OUT).read() == ffi_rs


def message(who):
    msg = _ffi.lib().pcv_last_error().decode()
    assert who + ": " in msg, msg
    return msg[msg.index(who + ": "):]


def test_bad_arguments_are_invalid_without_a_gpu():
    lib = _ffi.lib()
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    want = np.zeros((3, 8), dtype=np.float32)
    ids = np.zeros((2, 4), dtype=np.int64)
    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    good_w, good_a = i64(0, 2, 3), i64(0, 0, 1)

    def call(s=fake, k=4, pool=128, mode=0, lam=1.0, w=want, w_off=good_w, a=want, a_off=good_a, n=2):
        p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return lib.pcv_searcher_search_compound(s, None, 0, k, pool, mode, lam, p(w), p(w_off), p(a), p(a_off), n, p(ids), None, None, None, None, None, None)

    def refused(text, **kw):
        assert call(**kw) == PCV_ERR_INVALID
        assert message("search_compound").startswith("search_compound: " + text), message("search_compound")

    refused("searcher is NULL", s=None)
    for n in (0, -2):
        refused("n_compounds %d outside" % n, n=n)
    for k in (0, -1, PCV_MAX_RESULTS + 1, 1 << 20):
        refused("num_results %d outside [1,%d]" % (k, PCV_MAX_RESULTS), k=k, pool=4096)
    for k, pool in ((4, 3), (4, 0), (4, -5), (4, 4097), (128, 127)):
        refused("pool %d outside" % pool, k=k, pool=pool)
    for mode in (-1, 2, 7):
        refused("unknown mode %d" % mode, mode=mode)
    for lam in (-0.5, -1e-30, np.nan, np.inf, -np.inf):
        refused("avoid_weight", lam=lam)
    assert call(lam=0.0, s=None) == PCV_ERR_INVALID and message("search_compound").startswith("search_compound: searcher is NULL")  # (0 is a weight)
    refused("want_offsets is NULL", w_off=None)
    refused("want_offsets[0] must be 0", w_off=i64(1, 2, 3))
    refused("want_offsets are not ascending", w_off=i64(0, 2, 1))
    refused("compound 1 has 0 want vectors, outside [1,8]", w_off=i64(0, 2, 2))
    refused("compound 0 has 9 want vectors, outside [1,8]", w_off=i64(0, 9, 10))
    refused("want is NULL", w=None)
    refused("avoid is given without avoid_offsets", a_off=None)
    refused("avoid is NULL with 1 avoided vectors", a=None)
    refused("avoid_offsets[0] must be 0", a_off=i64(2, 2, 3))
    refused("avoid_offsets are not ascending", a_off=i64(0, 3, 1))
    refused("compound 1 has 9 avoid vectors, outside [0,8]", a_off=i64(0, 0, 9))
    # ... and the like form asks the same, then what pcv_searcher_search_like asks of its examples
    ex = i64(5, 6, 7)

    def like(s=fake, k=4, pool=128, mode=0, lam=1.0, w_ids=ex, w_w=None, w_ex=i64(0, 1, 2, 3), w_off=good_w, a_ids=ex, a_ex=i64(0, 3), a_off=good_a, n=2):
        p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return lib.pcv_searcher_search_compound_like(s, None, 0, k, pool, mode, lam, p(w_ids), p(w_w), p(w_ex), p(w_off), p(a_ids), None, p(a_ex), p(a_off),
                                                     n, 1, p(ids), None, None, None, None, None, None)

    def like_refused(text, **kw):
        assert like(**kw) == PCV_ERR_INVALID
        assert message("search_compound_like").startswith("search_compound_like: " + text), message("search_compound_like")

    like_refused("searcher is NULL", s=None)
    like_refused("n_compounds 0 outside", n=0)
    like_refused("num_results 0 outside", k=0)
    like_refused("pool 3 outside", pool=3)
    like_refused("unknown mode 2", mode=2)
    like_refused("avoid_weight", lam=-1.0)
    like_refused("want_offsets is NULL", w_off=None)
    like_refused("compound 0 has 9 want vectors", w_off=i64(0, 9, 10))
    like_refused("offsets is NULL", w_ex=None)
    like_refused("offsets[0] must be 0", w_ex=i64(1, 1, 2, 3))
    like_refused("offsets are not ascending", w_ex=i64(0, 2, 1, 3))
    like_refused("example ids NULL with 3 examples", w_ids=None)
    like_refused("weight 1 is not finite", w_w=np.array([1.0, np.nan, 1.0], dtype=np.float32))
    like_refused("the avoided side must be given whole", a_ex=None)
    like_refused("the avoided side must be given whole", a_off=None)
    like_refused("compound 1 has 9 avoid vectors", a_off=i64(0, 0, 9))


def test_python_packing_of_the_offsets():
    for name in ("search_compound", "search_compound_like_items"):
        assert callable(getattr(pa.Searcher, name)) and getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)
    a, b, c = np.arange(12, dtype=np.float32).reshape(3, 4), np.full(4, 7.0), np.zeros((0, 4))
    vec, off = pa.Searcher._compound_side([a, b, c, a[:2]], 4)
    assert off.tolist() == [0, 3, 4, 4, 6] and off.dtype == np.int64 and vec.dtype == np.float32 and vec.shape == (6, 4) and vec.flags.c_contiguous
    np.testing.assert_array_equal(vec, np.concatenate([a, b[None, :], a[:2]]))
    assert pa.Searcher._compound_side(None, 4) == (None, None)
    vec, off = pa.Searcher._compound_side([], 4)
    assert off.tolist() == [0] and vec.shape == (0, 4)
    with pytest.raises(ValueError):
        pa.Searcher._compound_side([np.zeros(5)], 4)
    assert [pa.Searcher._compound_mode(m) for m in ("all", "any", 0, 1, 5)] == [0, 1, 0, 1, 5]
    ids, w, ex, off = pa.Searcher._compound_like_side([[[1, 2], [3]], [[(4, 0.5), (5, 2.0), 6]]])
    assert ids.tolist() == [1, 2, 3, 4, 5, 6] and w.tolist() == [1.0, 1.0, 1.0, 0.5, 2.0, 1.0] and ex.tolist() == [0, 2, 3, 6] and off.tolist() == [0, 2, 3]
    assert ids.dtype == ex.dtype == off.dtype == np.int64 and w.dtype == np.float32
    ids, w, ex, off = pa.Searcher._compound_like_side([[[9]], []])
    assert ex.tolist() == [0, 1] and off.tolist() == [0, 1, 1]  # (a compound without parts: the library refuses it)
    assert pa.Searcher._compound_like_side(None) == (None, None, None, None)
    out = pa.Searcher._compound_outputs(3, 5)
    assert [o.shape for o in out] == [(3, 5), (3, 5), (3, 5, 8), (3, 5), (3,), (3,), (3,)]
    assert [o.dtype for o in out] == [np.int64, np.float64, np.float32, np.float64, np.int32, np.int32, np.uint8]


def test_rust_and_cpp_surfaces_reach_the_calls():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    m = re.search(r"pub fn search_compound\((.*?)\n    }\n", search_rs, flags=re.S)
    assert m and "ffi::pcv_searcher_search_compound(" in m.group(1) and "ffi::PCV_MAX_COMPOUND_POOL" in m.group(1)
    assert "ffi::PCV_COMPOUND_ALL" in search_rs and "ffi::PCV_COMPOUND_ANY" in search_rs
    m = re.search(r"pub fn search_compound_like_items\((.*?)\n    }\n", search_rs, flags=re.S)
    assert m and "ffi::pcv_searcher_search_compound_like(" in m.group(1)
    assert search_rs.index("pub fn search_compound(") < search_rs.index("impl Drop for Searcher")
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    assert hpp.count("search_compound(") >= 2 and "pcv_searcher_search_compound(" in hpp and "pcv_searcher_search_compound_like(" in hpp
    assert "struct Compound {" in hpp and "struct CompoundItem {" in hpp
    src = os.path.join(ROOT, "tests", "cpp", "compound_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "compound_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


# ---- the model on hand-made lists --------------------------------------------------------------------------------------------------
class FakeOracle:
    """scores[v][row]: canonical scores given outright (NaN: the row is not listed); ties -> lower position"""

    def __init__(self, scores):
        self.scores = np.asarray(scores, dtype=np.float64)

    def topk(self, queries, rows, k, metric=0):
        V, n = self.scores.shape
        pos = np.full((V, k), -1, np.int64)
        sc = np.full((V, k), np.nan, np.float64)
        cnt = np.zeros(V, np.int32)
        for v in range(V):
            listed = [x for x in range(n) if not np.isnan(self.scores[v, x])]
            listed.sort(key=lambda x: (-self.scores[v, x], x))
            cnt[v] = len(listed)
            pos[v, :len(listed)] = listed
            sc[v, :len(listed)] = self.scores[v, listed]
        return pos, sc, cnt


def make_ref(scores, metric="cosine", dim=4):
    scores = np.asarray(scores, dtype=np.float64)
    n = scores.shape[1]
    return cr.CompoundReference(FakeOracle(scores), np.zeros((scores.shape[0], dim), np.float32), np.zeros((n, dim), np.float32),
                                np.arange(n, dtype=np.int64) * 10 + 5, metric)


def test_model_on_hand_made_lists():
    # six rows, three vectors; every number a dyadic fraction, so the arithmetic is exact
    A = [0.875, 0.75, 0.25, 0.5, 0.125, 0.0]
    B = [0.125, 0.5, 0.75, 0.5, 0.875, 0.0]
    N = [0.5, -0.25, 0.0, 0.25, 0.0, 0.75]
    ref = make_ref([A, B, N])
    # ALL: min(A, B) = .125 .5 .25 .5 .125 0 -> rows 1 and 3 tie at 0.5 (position decides), then 2, then 0 and 4 tie
    w = ref.brute((0, 1), (), ALL, 1.0, 6)
    assert w.pos.tolist() == [1, 3, 2, 0, 4, 5] and w.combined.tolist() == [0.5, 0.5, 0.25, 0.125, 0.125, 0.0] and w.penalties.tolist() == [0.0] * 6
    assert w.ids.tolist() == [15, 35, 25, 5, 45, 55]
    np.testing.assert_array_equal(w.parts[:, :2], np.array([[A[x], B[x]] for x in w.pos], dtype=np.float32))
    assert np.isnan(w.parts[:, 2:]).all()
    # ANY: max(A, B) = .875 .75 .75 .5 .875 0
    assert ref.brute((0, 1), (), ANY, 1.0, 6).pos.tolist() == [0, 4, 1, 2, 3, 5]
    # the hinge: only rows that resemble N pay — row 1 (N = -0.25) pays nothing, row 3 pays 0.5 * 0.25
    w = ref.brute((0, 1), (2,), ALL, 0.5, 6)
    assert w.penalties.tolist() == [0.0, 0.125, 0.0, 0.0, 0.25, 0.375] and w.pos.tolist() == [1, 3, 2, 4, 0, 5]
    assert w.combined.tolist() == [0.5, 0.375, 0.25, 0.125, -0.125, -0.375]
    # lambda = 0 with avoided vectors present is the compound without them
    a, b = ref.brute((0, 1), (2,), ALL, 0.0, 6), ref.brute((0, 1), (), ALL, 0.0, 6)
    assert a.pos.tolist() == b.pos.tolist() and cr.bits64(a.combined).tolist() == cr.bits64(b.combined).tolist()
    # W = 1 is the plain list, and the same vector twice is the same again, no row twice
    assert ref.brute((0,), (), ALL, 1.0, 6).pos.tolist() == ref.brute((0,), (), ANY, 1.0, 6).pos.tolist() == [0, 1, 3, 2, 4, 5]
    assert ref.walk((0, 0), (), ALL, 1.0, 6, 128).pos.tolist() == [0, 1, 3, 2, 4, 5]
    # a walk over lists shorter than a step ends with the lists: exact, examined = their length
    w = ref.walk((0, 1), (), ALL, 1.0, 2, 128)
    assert (w.pos.tolist(), w.examined, w.exact) == ([1, 3], 6, True)
    # a row without a score under one vector is no candidate, and shortens that list
    C_ = [0.5, np.nan, 0.25, 0.125, 0.0, 0.0]
    ref2 = make_ref([A, C_])
    w = ref2.walk((0, 1), (), ANY, 1.0, 6, 128)
    assert 1 not in w.pos.tolist() and len(w.pos) == 5 and w.exact and w.examined == 6
    # the dot metric: rel = c / dim, one division
    d = make_ref([[3.0, 1.0], [1.0, 2.0]], metric="dot", dim=3)
    w = d.brute((0, 1), (), ALL, 1.0, 2)
    assert w.pos.tolist() == [0, 1] and cr.bits64(w.combined).tolist() == cr.bits64(np.array([F64(1.0) / F64(3.0), F64(1.0) / F64(3.0)])).tolist()
    np.testing.assert_array_equal(w.parts[0, :2], cr.reported([3.0, 1.0], "dot", 3))


def stepped(n, top, step=2.0 ** -12):
    """a list of n falling scores from `top`, exact in f64"""
    return [top - r * step for r in range(n)]


def test_walk_in_steps_the_certificate_is_strict():
    n = 400
    # vector 0 ranks the rows 0, 1, 2 ...; vector 1 ranks them n-1, n-2, ...: ALL's best rows are in the middle of both lists
    a = stepped(n, 0.5)
    b = list(reversed(a))
    ref = make_ref([a, b])
    m = [min(x, y) for x, y in zip(a, b)]
    best = sorted(range(n), key=lambda x: (-m[x], x))
    for k, pool in ((1, 4096), (4, 4096), (4, 128), (4, 200), (4, 256)):
        w = ref.walk((0, 1), (), ALL, 1.0, k, pool)
        # after e entries of each list the bound is a[e - 1]; row 199 (m = a[200]) and row 200 (m = a[200]) are met at e = 200, 201
        if pool >= 256:
            assert w.exact and w.examined == 256 and w.pos.tolist() == best[:k] == ref.brute((0, 1), (), ALL, 1.0, k).pos.tolist()
        else:
            assert not w.exact and w.examined == pool
    # (with pool 200 every row has been met — row 199 in one list, row 200 in the other — and the answer is the right one, but the bound
    # a[199] is above it: a 0 is no disproof)
    assert ref.walk((0, 1), (), ALL, 1.0, 4, 200).pos.tolist() == best[:4]
    # ANY certifies at once: the k-th best of the union lies above both lists' 128th entries
    w = ref.walk((0, 1), (), ANY, 1.0, 10, 4096)
    assert w.exact and w.examined == 128 and w.pos.tolist() == ref.brute((0, 1), (), ANY, 1.0, 10).pos.tolist()
    # a tie at the bound: one list, k = 128 — the last kept row IS the last entry walked, m == T, and that does not certify ...
    one = make_ref([stepped(n, 0.5)])
    w = one.walk((0,), (), ALL, 1.0, 128, 128)
    assert (w.examined, w.exact) == (128, False) and w.pos.tolist() == list(range(128))
    w = one.walk((0,), (), ALL, 1.0, 128, 4096)  # ... the next step does
    assert (w.examined, w.exact) == (256, True) and w.pos.tolist() == list(range(128))
    assert one.walk((0,), (), ALL, 1.0, 127, 128).exact  # (m_127 = a[126] > a[127])
    # ... and it must not: rows 127 and 128 score the same under vector 0, row 128 is far better under vector 1; with the lists
    # [.., 127, 128, ..] the bound after 128 entries equals m of row 127, and the unmet row 128 has the same m: relaxing the test to
    # >= would certify an answer that depends on nothing but luck; the strict test walks on and finds that the kept row stays (lower
    # position), a claim the first step could not make
    a = stepped(n, 0.5)
    a[128] = a[127]
    tie = make_ref([a, [1.0] * n])
    w = tie.walk((0, 1), (), ALL, 1.0, 128, 128)
    assert float(w.combined[-1]) == a[127] and not w.exact
    w = tie.walk((0, 1), (), ALL, 1.0, 128, 4096)
    assert w.exact and w.examined == 256 and w.pos.tolist() == tie.brute((0, 1), (), ALL, 1.0, 128).pos.tolist() == list(range(128))
    # pool 129: the second step asks for one entry; the end of a list inside a step is exact
    w = one.walk((0,), (), ALL, 1.0, 10, 129)
    assert (w.examined, w.exact) == (128, True)
    # |L| == pool == 129: the second step gets the one entry it asks for, and m_128 = a[127] > T = a[128] certifies
    short = make_ref([stepped(129, 0.5)])
    w = short.walk((0,), (), ALL, 1.0, 128, 129)
    assert (w.examined, w.exact) == (129, True)
    w = short.walk((0,), (), ALL, 1.0, 128, 4096)  # ... as does the end of the list
    assert (w.examined, w.exact) == (129, True)


@pytest.fixture(scope="module")
def shared(oracle):
    from test_distinct_gpu import planted_corpus, planted_queries

    out = {}
    for metric in ("cosine", "dot"):
        rows, ids, anchors, bridge_ids = cr.bridged_corpus(planted_corpus, metric)
        vectors = cr.compound_vectors(planted_queries, metric, anchors)
        out[metric] = (rows, ids, vectors, bridge_ids, cr.CompoundReference(oracle, vectors, rows, ids, metric))
    return out


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_the_shared_inputs_reach_every_branch(shared, metric):
    """(what test_compound_gpu.py relies on, from the model alone) some compounds certify in the first pass, some need more than one,
    some end at the pool uncertified; every exact walk is the brute force; the bridge rows answer ALL of a pair of neighbours."""
    rows, ids, _vectors, bridge_ids, ref = shared[metric]
    first = later = ended = 0
    for want, avoid in cr.COMPOUNDS + cr.COMPOUNDS_W8:
        for mode in (ALL, ANY):
            for lam in (cr.LAMBDAS if avoid else (0.5,)):
                for k, pool in ((10, 128), (10, 4096), (128, 300), (128, 4096), (1, 1)):
                    w = ref.walk(want, avoid, mode, lam, k, pool)
                    first += w.exact and w.examined <= 128
                    later += w.exact and w.examined > 128
                    ended += not w.exact
                    if w.exact:
                        b = ref.brute(want, avoid, mode, lam, k)
                        assert w.pos.tolist() == b.pos.tolist() and cr.bits64(w.combined).tolist() == cr.bits64(b.combined).tolist()
    print(metric, "first pass", first, "later", later, "at the pool", ended)
    assert first >= 20 and later >= 20 and ended >= 20
    # (the rows planted near anchors 0 AND 1: the pair's family and — the amplitudes of the dot metric mix them — the two wider ones)
    near_both = set(np.concatenate([b for tup, b in zip(cr.BRIDGES, bridge_ids) if 0 in tup and 1 in tup]).tolist())
    w = ref.walk((0, 1), (), ALL, 1.0, 10, 128)
    assert w.exact and w.examined == 128 and set(w.ids.tolist()) <= near_both
    assert not set(ref.walk((0, 1), (), ANY, 1.0, 10, 128).ids.tolist()) & near_both
