"""CPU: the group-aware pair calls (pcv_searcher_neighbors_grouped, _match_grouped, _find_duplicates_grouped,
_last_pair_group_stats) are declared, exported, bound and present in the regenerated Rust ffi; every PCV_ERR_INVALID case needs no GPU;
the Python, C++ and Rust surfaces reach the calls; and the reference the GPU tests compare with (pair_groups_ref.py) agrees with the
definition itself on small inputs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_ref
import neighbors_ref
import pair_groups_ref as ref
import perceive_amd as pa
from duplicates_ref import bits
from perceive_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCV_ERR_INVALID = 1  # include/perceive_hip.h
ARITY = {"pcv_searcher_neighbors_grouped": 12, "pcv_searcher_match_grouped": 15, "pcv_searcher_find_duplicates_grouped": 11,
         "pcv_searcher_last_pair_group_stats": 2}
STATS = [("grouped_rows", "int64_t"), ("sibling_candidates", "int64_t"), ("collapsed", "int64_t"), ("flags", "uint32_t"),
         ("bound_tile_rows", "int32_t"), ("groups_ms", "float")]


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "perceive_hip.h")).read(), flags=re.S)


def test_declared_exported_and_bound():
    h = header()
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pcv_[a-z0-9_]+)", out))
    lib = _ffi.lib()
    for name, arity in ARITY.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, h, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == arity
        assert name in exported
        assert name in _ffi.SYMBOLS and getattr(lib, name).argtypes
        assert len(_ffi.SYMBOLS[name][1]) == arity
    assert re.search(r"enum \{ PCV_GROUPS_SKIP_OWN = 1, PCV_GROUPS_ONE_PER_GROUP = 2 \};", h)
    assert (pa.GROUPS_SKIP_OWN, pa.GROUPS_ONE_PER_GROUP) == (1, 2) == (ref.SKIP_OWN, ref.ONE_PER_GROUP)
    m = re.search(r"typedef struct pcv_pair_group_stats \{(.*?)\} pcv_pair_group_stats;", h, flags=re.S)
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    assert fields == STATS
    assert [(n, widths[t]) for n, t in fields] == list(_ffi.PairGroupStats._fields_)
    assert C.sizeof(_ffi.PairGroupStats) == 40  # no padding
    # the flags sit where the issue puts them: behind k / min_score, in front of capacity; the groups behind the scores
    for name, before, after in (("pcv_searcher_neighbors_grouped", "int k", "int64_t capacity"), ("pcv_searcher_match_grouped", "float min_score", "int64_t capacity")):
        params = [" ".join(x.split()) for x in re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, h, flags=re.S).group(1).split(",")]
        i = params.index("uint32_t flags")
        assert params[i - 1] == before and params[i + 1] == after
        j = params.index("float* out_scores")
        assert params[j + 1].startswith("int64_t* out_") and params[j + 1].endswith("_groups") and params[j + 2] == "int32_t* out_counts"
    # the plain signatures are as they were
    assert re.search(r"pcv_searcher_neighbors\(pcv_searcher\* s, const int64_t\* source_ids, int n_sources, int k, int64_t capacity, int64_t\* out_ids,", h)
    assert len(re.search(r"\bpcv_searcher_match\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1).split(",")) == 13
    assert len(re.search(r"\bpcv_searcher_find_duplicates\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1).split(",")) == 10


def test_regenerated_rust_ffi_is_current():
    ffi_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "ffi.rs")).read()
    assert ("pub fn pcv_searcher_neighbors_grouped(s: *mut pcv_searcher, source_ids: *const i64, n_sources: c_int, k: c_int, flags: u32, capacity: i64, "
            "out_ids: *mut i64, out_neighbor_ids: *mut i64, out_scores: *mut f32, out_neighbor_groups: *mut i64, out_counts: *mut i32, "
            "out_rows: *mut i64) -> c_int;") in ffi_rs
    assert "min_score: f32, flags: u32, capacity: i64, out_ids: *mut i64, out_match_ids: *mut i64, out_scores: *mut f32, out_match_groups: *mut i64," in ffi_rs
    assert "out_count: *mut i64, out_total: *mut i64, out_skipped: *mut i64) -> c_int;" in ffi_rs
    assert "pub fn pcv_searcher_last_pair_group_stats(s: *mut pcv_searcher, out: *mut pcv_pair_group_stats) -> c_int;" in ffi_rs
    assert "pub const PCV_GROUPS_SKIP_OWN: c_int = 1;" in ffi_rs and "pub const PCV_GROUPS_ONE_PER_GROUP: c_int = 2;" in ffi_rs
    rust = {"int64_t": "i64", "int32_t": "i32", "uint32_t": "u32", "float": "f32"}
    want = r"pub struct pcv_pair_group_stats \{\s*" + r"\s*".join(r"pub %s: %s," % (n, rust[t]) for n, t in STATS) + r"\s*\}"
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
    ids = np.full(4, -77, dtype=np.int64)
    nbr = np.full((4, 64), -77, dtype=np.int64)
    grp = np.full((4, 64), -77, dtype=np.int64)
    scores = np.full((4, 64), -77, dtype=np.float32)
    counts = np.full(4, -77, dtype=np.int32)
    rows = C.c_int64(-5)
    arrays = dict(ids_p=_ffi.i64p(ids), nbr_p=_ffi.i64p(nbr), scores_p=_ffi.f32p(scores), counts_p=_ffi.i32p(counts))
    nothing = dict(capacity=0, ids_p=None, nbr_p=None, scores_p=None, counts_p=None, grp_p=None)

    def nb(s, k=3, flags=1, capacity=4, rows_p=C.byref(rows), grp_p=_ffi.i64p(grp), **kw):
        a = dict(arrays, **kw)
        return lib.pcv_searcher_neighbors_grouped(s, None, 0, k, flags, capacity, a["ids_p"], a["nbr_p"], a["scores_p"], grp_p, a["counts_p"], rows_p)

    def mt(s, k=3, min_score=-1.0, flags=1, capacity=4, rows_p=C.byref(rows), grp_p=_ffi.i64p(grp), **kw):
        a = dict(arrays, **kw)
        return lib.pcv_searcher_match_grouped(s, None, 0, None, 0, k, min_score, flags, capacity, a["ids_p"], a["nbr_p"], a["scores_p"], grp_p,
                                              a["counts_p"], rows_p)

    def message(word):
        msg = lib.pcv_last_error().decode()
        assert word in msg
        return msg

    for call, word in ((nb, "neighbors_grouped"), (mt, "match_grouped")):
        # the flags come before everything, the handle included
        for flags in (4, 5, 8, 0x80000000, 0xFFFFFFFF):
            assert call(None, flags=flags) == PCV_ERR_INVALID
            assert "outside 0..3" in message(word)
            assert call(fake, flags=flags, k=0, capacity=-1, rows_p=None) == PCV_ERR_INVALID
            assert "outside 0..3" in message(word)
        for flags in (0, 1, 2, 3):  # legal flags: every other rule is the plain call's, in its order
            assert call(None, flags=flags) == PCV_ERR_INVALID
            assert "searcher is NULL" in message(word)
            assert call(fake, flags=flags, rows_p=None) == PCV_ERR_INVALID
            assert "out_rows is NULL" in message(word)
        for k in (0, -1, 65, 1 << 20):
            assert call(fake, k=k) == PCV_ERR_INVALID
            assert "k %d outside [1,64]" % k in message(word)
            assert call(fake, k=k, **nothing) == PCV_ERR_INVALID
        for cap in (-1, -(1 << 40)):
            assert call(fake, capacity=cap) == PCV_ERR_INVALID
            assert "capacity %d is negative" % cap in message(word)
        for name in arrays:
            assert call(fake, **{name: None}) == PCV_ERR_INVALID
            assert "is NULL with capacity 4" in message(word)
            assert call(fake, capacity=0, **{name: None}) == PCV_ERR_INVALID  # counting only means every array NULL
        assert call(fake, **dict(nothing, grp_p=_ffi.i64p(grp))) == PCV_ERR_INVALID  # ... the groups too
        assert call(None, **nothing) == PCV_ERR_INVALID
        assert "searcher is NULL" in message(word)
    assert mt(fake, min_score=float("nan")) == PCV_ERR_INVALID
    assert "min_score is NaN" in message("match_grouped")
    for lo in (-1.0000001, 1.0000001, -2.0, float("inf")):
        assert mt(fake, min_score=lo) == PCV_ERR_INVALID
        assert "outside [-1, 1]" in message("match_grouped")
    assert mt(fake, k=0, min_score=float("nan"), capacity=-1) == PCV_ERR_INVALID  # the order of the checks: k, min_score, capacity
    assert "k 0 outside" in message("match_grouped")
    assert rows.value == -5  # nothing was written
    assert (ids == -77).all() and (nbr == -77).all() and (grp == -77).all() and (scores == -77).all() and (counts == -77).all()

    # find_duplicates_grouped: the plain call's rules, no flags
    a = np.full(8, -77, dtype=np.int64)
    b = np.full(8, -77, dtype=np.int64)
    sc = np.full(8, -77, dtype=np.float32)
    count, total, skipped = C.c_int64(-5), C.c_int64(-5), C.c_int64(-5)

    def dup(s, threshold=0.9, max_pairs=8, a_p=_ffi.i64p(a), b_p=_ffi.i64p(b), count_p=C.byref(count)):
        return lib.pcv_searcher_find_duplicates_grouped(s, None, 0, threshold, max_pairs, a_p, b_p, _ffi.f32p(sc), count_p, C.byref(total), C.byref(skipped))

    assert dup(None) == PCV_ERR_INVALID
    assert "searcher is NULL" in message("find_duplicates_grouped")
    for kw in (dict(a_p=None), dict(b_p=None), dict(count_p=None)):
        assert dup(fake, **kw) == PCV_ERR_INVALID
        assert "is NULL" in message("find_duplicates_grouped")
    for m in (0, -1, (1 << 24) + 1):
        assert dup(fake, max_pairs=m) == PCV_ERR_INVALID
        assert "max_pairs %d outside" % m in message("find_duplicates_grouped")
    assert dup(fake, threshold=float("nan")) == PCV_ERR_INVALID
    assert "threshold is NaN" in message("find_duplicates_grouped")
    for t in (-1.0, -1.5, 1.0000001, float("inf")):
        assert dup(fake, threshold=t) == PCV_ERR_INVALID
        assert "outside (-1, 1]" in message("find_duplicates_grouped")
    assert (count.value, total.value, skipped.value) == (-5, -5, -5) and (a == -77).all() and (b == -77).all() and (sc == -77).all()
    st = _ffi.PairGroupStats()
    assert lib.pcv_searcher_last_pair_group_stats(None, C.byref(st)) == PCV_ERR_INVALID
    assert lib.pcv_searcher_last_pair_group_stats(fake, None) == PCV_ERR_INVALID
    assert b"last_pair_group_stats" in lib.pcv_last_error()


def test_python_surface():
    names = ("neighbors_grouped", "match_grouped", "find_duplicates_grouped", "last_pair_group_stats")
    for cls in (pa.Searcher, pa.SearcherView):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    for name in names:
        assert getattr(pa.SearcherView, name) is getattr(pa.Searcher, name)  # inherited
    src = open(os.path.join(ROOT, "perceive_amd", "search.py")).read()
    body = src[src.index("    def neighbors_grouped("):src.index("    def last_pair_group_stats(")]
    for call in ("pcv_searcher_neighbors_grouped(", "pcv_searcher_match_grouped("):
        assert body.count(call) == 2  # the count, then the table
    assert body.count("pcv_searcher_find_duplicates_grouped(") == 1
    # the mirror only converts arguments: no arithmetic on rows or scores, no filtering on the host, no other call of the library
    assert body.count("_ffi.lib().") == 5
    code = re.sub(r'""".*?"""', "", body, flags=re.S)  # (without the docstrings)
    for word in (".neighbors(", ".match(", ".find_duplicates(", "groups_of", "np.sort", "argsort", "np.where", " for ", " while "):
        assert word not in code, word
    # the existing methods keep their signatures
    import inspect

    assert list(inspect.signature(pa.Searcher.neighbors).parameters) == ["self", "sources", "k"]
    assert list(inspect.signature(pa.Searcher.match).parameters) == ["self", "from_sources", "to_sources", "k", "min_score"]
    assert list(inspect.signature(pa.Searcher.find_duplicates).parameters) == ["self", "sources", "threshold", "max_pairs"]


def test_rust_shim_declares_and_calls_it():
    search_rs = open(os.path.join(ROOT, "shim", "perceive-core", "src", "search.rs")).read()
    for fn, sym, n in (("neighbors_grouped", "pcv_searcher_neighbors_grouped", 2), ("matches_grouped", "pcv_searcher_match_grouped", 2),
                       ("find_duplicates_grouped", "pcv_searcher_find_duplicates_grouped", 1), ("last_pair_group_stats", "pcv_searcher_last_pair_group_stats", 1)):
        m = re.search(r"pub fn %s\(&self.*?\n    }\n" % fn, search_rs, flags=re.S)
        assert m, fn
        assert m.group(0).count("ffi::%s(" % sym) == n
        assert search_rs.index("pub fn %s(" % fn) < search_rs.index("impl Drop for Searcher")


def test_cpp_mirror_pair_groups_program_compiles():
    hpp = open(os.path.join(ROOT, "include", "perceive.hpp")).read()
    for method, sym, calls in ((" neighbors_grouped(", "pcv_searcher_neighbors_grouped(", 2), (" match_grouped(", "pcv_searcher_match_grouped(", 2),
                               (" find_duplicates_grouped(", "pcv_searcher_find_duplicates_grouped(", 1),
                               (" last_pair_group_stats(", "pcv_searcher_last_pair_group_stats(", 2)):
        assert hpp.count(method) == 2 and hpp.count(sym) == calls, method  # Searcher and SearcherView
    src = os.path.join(ROOT, "tests", "cpp", "pair_groups_mirror_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "pair_groups_mirror_test.bin")
    subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
         "-L" + os.path.join(ROOT, "perceive_amd"), "-lperceive_hip", "-Wl,-rpath," + os.path.join(ROOT, "perceive_amd")],
        check=True, capture_output=True, text=True)
    assert os.path.exists(out)


# ---- the reference against the definition -------------------------------------------------------------------------------------------
def small(golden_dir, name, n, sizes, seed):
    """n rows of a golden corpus with: groups of the given sizes handed out in a shuffled order (the rest ungrouped), a tie across two
    groups and a singleton, two ungrouped rows that share an id, two grouped rows that share an id, and the rows that keep their place:
    a zero row, a hidden row, a repeated id."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    rows = np.array(g["corpus"], dtype=np.float32)[:n].copy()
    rng = np.random.default_rng(seed)
    ids = (rng.permutation(n) * 5 + 300).astype(np.int64)
    order = rng.permutation(n)
    table, at = {}, 0
    for key, size in enumerate(sizes):
        for r in order[at : at + size]:
            table[int(ids[r])] = 1000 + key
        at += size
    free = [int(r) for r in order[at:]]  # ungrouped rows
    grouped = [int(r) for r in order[:at]]
    # ties across groups: one vector at three positions — a member of group 1000, a member of another group, an ungrouped row
    a = grouped[0]
    b = next(r for r in grouped if table[int(ids[r])] != table[int(ids[a])])
    rows[b] = rows[a] * np.float32(2.0)
    rows[free[0]] = rows[a] * np.float32(0.5)
    rows[free[5]] = rows[a] + np.float32(0.05) * rows[free[5]]  # an ungrouped owner for which the three are the best partners
    ids[free[2]] = ids[free[1]]      # two ungrouped rows share an id: not siblings
    ids[grouped[-1]] = ids[grouped[-2]]  # two rows share an id with a group: siblings (the one takes the other's group)
    rows[free[3]] = 0.0               # no cosine
    part = np.ones(n, dtype=bool)
    part[[free[4], grouped[-4]]] = False  # hidden
    groups = ref.row_groups(ids, table)
    assert groups[free[1]] == groups[free[2]] == -1 and groups[grouped[-1]] == groups[grouped[-2]] >= 0
    assert len({a, b, grouped[-1], grouped[-2], grouped[-4]}) == 5
    return np.ascontiguousarray(rows), ids, groups, part, a, b, free[0]


CASES = [("scan_n77_d100", 77, (1, 2, 8, 50), 1), ("scan_n77_d100", 60, (2, 2, 2, 8, 8, 1, 1), 2), ("scan_n1000_d384", 90, (50, 8, 8, 2, 1), 3)]


def corpus16(seed=16):
    """200 rows of 16 features: low dimension, many near ties of the f64 cosines' leading digits"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-2, 3, size=(200, 16)).astype(np.float32)  # small integers: exact ties are common
    rows[rows.any(axis=1) == 0] = 1.0
    ids = (rng.permutation(200) * 3 + 7).astype(np.int64)
    groups = np.where(rng.random(200) < 0.8, rng.integers(0, 12, size=200), -1).astype(np.int64)
    groups[:50] = 99  # a group of 50
    part = rng.random(200) > 0.05
    return rows, ids, groups, part


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_reference_is_the_definition(oracle, golden_dir, case, flags):
    name, n, sizes, seed = CASES[case]
    rows, ids, groups, part, a, b, c = small(golden_dir, name, n, sizes, seed)
    live = neighbors_ref.takes_part(rows, part)
    assert live[[a, b, c]].all() and not live.all()
    for k in (1, 4, 64):
        want = ref.brute_force(oracle, rows, ids, groups, k, flags, part=part)
        got = ref.reference(oracle, rows, ids, groups, k, flags, part=part)
        ref.check(got, want)
        used = np.arange(k)[None, :] < want[4][:, None]
        assert (want[4][~live] == 0).all() and (want[3][~used] == -1).all() and (want[1][~used] == -1).all()
        pos_of = {}
        for r in range(n):
            pos_of.setdefault(int(ids[r]), []).append(r)
        for r in np.nonzero(live)[0]:
            gk = want[3][r, : want[4][r]]
            if flags & ref.SKIP_OWN and groups[r] >= 0:
                assert (gk != groups[r]).all()
            if flags & ref.ONE_PER_GROUP:
                assert len(set(gk[gk >= 0].tolist())) == int((gk >= 0).sum())
    if flags == 0:  # the plain reference
        for k in (1, 4, 64):
            plain = neighbors_ref.reference(oracle, rows, ids, k, part)
            got = ref.reference(oracle, rows, ids, groups, k, 0, part=part)
            ref.check(got, plain[:3] + (got[3], plain[3]))
    # the tie: a, b = 2a and c = a / 2 have one cosine with every owner; position decides, and b collapses into a only if they share a group
    owner = next(int(r) for r in np.nonzero(live)[0] if r not in (a, b, c) and groups[r] == -1 and
                 neighbors_ref.reference(oracle, rows, ids, 1, part)[2][r, 0] > 0.9)
    got = ref.reference(oracle, rows, ids, groups, 64, flags, part=part)
    listed = got[1][owner, : got[4][owner]].tolist()
    trio = sorted((a, b, c))
    at = [listed.index(int(ids[r])) for r in trio]
    assert at == [0, 1, 2]  # all three are kept (different groups, or none), adjacent, in position order
    assert len({bits(got[2][owner, i : i + 1])[0] for i in at}) == 1


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_reference_low_dimension_and_match(oracle, flags):
    rows, ids, groups, part = corpus16()
    for k in (1, 10, 64):
        ref.check(ref.reference(oracle, rows, ids, groups, k, flags, part=part), ref.brute_force(oracle, rows, ids, groups, k, flags, part=part))
    # rectangles with a score bound: owners behind the partners and in front of them, overlapping
    src = np.repeat([0, 1, 2], [70, 60, 70])
    for frm, to in (([0], [1, 2]), ([2], [0]), ([0, 1], [1, 2])):
        owner, partner = np.isin(src, frm), np.isin(src, to)
        for lo in (-1.0, 0.2):
            want = ref.brute_force(oracle, rows, ids, groups, 10, flags, owner, partner, lo, part)
            got = ref.reference(oracle, rows, ids, groups, 10, flags, owner, partner, lo, part)
            ref.check(got, want)
            if lo != -1.0:
                used = np.arange(10)[None, :] < want[4][:, None]
                assert (want[2][used].astype(np.float64) >= float(np.float32(lo)) - 1e-7).all() and want[4].min() < 10
    # flags 0 over a rectangle is the match reference
    owner, partner = np.isin(src, [0]), np.isin(src, [1, 2])
    plain = match_ref.reference(oracle, rows, ids, owner, partner, 10, 0.2, part)
    got = ref.reference(oracle, rows, ids, groups, 10, 0, owner, partner, 0.2, part)
    ref.check(got, plain[:3] + (got[3], plain[3]))


def test_duplicates_reference(oracle):
    import duplicates_ref

    rows, ids, groups, part = corpus16(5)
    rows[1], rows[3], rows[60] = rows[0], rows[2] * np.float32(2.0), rows[0]  # sibling pairs (rows 0..49 are one group) and a foreign copy
    part[[0, 1, 2, 3, 60]] = True
    groups[60] = 3
    pos = np.nonzero(part)[0]
    plain = duplicates_ref.reference(oracle, rows, ids, 0.8, pos)
    a, b, sc, skipped = ref.duplicates(oracle, rows, ids, groups, 0.8, pos)
    assert skipped > 0 and len(a) > 0 and len(a) + skipped == len(plain[0])
    # by the definition, pair by pair
    want = []
    for i in pos:
        for j in pos:
            if i < j and not (groups[i] >= 0 and groups[i] == groups[j]):
                c = oracle.canonical_score(rows[i], rows[j])
                if c >= float(np.float32(0.8)):
                    want.append((-c, int(i), int(j)))
    want.sort()
    assert [int(x) for x in a] == [int(ids[w[1]]) for w in want] and [int(x) for x in b] == [int(ids[w[2]]) for w in want]
    np.testing.assert_array_equal(bits(sc), bits(np.array([-w[0] for w in want], dtype=np.float64).astype(np.float32)))
    none = ref.duplicates(oracle, rows, ids, np.full(200, -1), 0.8, pos)
    assert none[3] == 0 and len(none[0]) == len(plain[0])
