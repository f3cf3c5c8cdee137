"""CPU: top-m labels (pcv_searcher_assign_top) without a device — the argument errors that come back before any device work, and the
reference the GPU tests compare with (assign_top_ref.py) against the definition itself."""
import ctypes as C
import os

import numpy as np
import pytest

from assign_ref import assign_reference
from assign_top_ref import assign_top_reference, bits, brute_force
from perceive_amd import _ffi

PCV_ERR_INVALID = 1


def test_argument_errors_without_a_device():
    L = _ffi.lib()
    lab = np.zeros((2, 8), dtype=np.float32)
    out = np.zeros(8, dtype=np.int32)
    cnt = np.zeros(4, dtype=np.int32)
    n = C.c_int64(-5)
    ninf = float("-inf")
    fake = C.c_void_p(0)  # no searcher: every check below comes before the handle is looked at
    tail = (None, None, None, None, None, C.byref(n))  # the count-only form
    assert L.pcv_searcher_assign_top(fake, None, 2, 1, ninf, None, 0, 0, *tail) == PCV_ERR_INVALID
    assert b"NULL" in L.pcv_last_error()
    assert L.pcv_searcher_assign_top(fake, _ffi.f32p(lab), 2, 1, ninf, None, 0, 0, None, None, None, None, None, None) == PCV_ERR_INVALID
    for k in (0, -1, 4097):
        assert L.pcv_searcher_assign_top(fake, _ffi.f32p(lab), k, 1, ninf, None, 0, 0, *tail) == PCV_ERR_INVALID
        assert b"outside [1,4096]" in L.pcv_last_error()
    for m in (0, -1, 9):
        assert L.pcv_searcher_assign_top(fake, _ffi.f32p(lab), 2, m, ninf, None, 0, 0, *tail) == PCV_ERR_INVALID
        assert b"outside [1,8]" in L.pcv_last_error()
    assert L.pcv_searcher_assign_top(fake, _ffi.f32p(lab), 2, 2, float("nan"), None, 0, 0, *tail) == PCV_ERR_INVALID
    assert b"NaN" in L.pcv_last_error()
    assert L.pcv_searcher_assign_top(fake, _ffi.f32p(lab), 2, 2, ninf, None, 0, 4, *tail) == PCV_ERR_INVALID  # no out_labels
    assert b"out_labels is NULL" in L.pcv_last_error()
    assert L.pcv_searcher_assign_top(fake, _ffi.f32p(lab), 2, 2, ninf, None, 0, -1, *tail) == PCV_ERR_INVALID
    assert L.pcv_searcher_assign_top(fake, _ffi.f32p(lab), 2, 2, ninf, None, 0, 4, _ffi.i32p(out), None, None, None, None, C.byref(n)) == PCV_ERR_INVALID
    assert b"out_counts is NULL" in L.pcv_last_error()
    assert L.pcv_searcher_assign_top(fake, _ffi.f32p(lab), 2, 2, 0.25, None, 0, 4, _ffi.i32p(out), None, None, _ffi.i32p(cnt), None, C.byref(n)) == PCV_ERR_INVALID
    assert b"searcher is NULL" in L.pcv_last_error()
    assert L.pcv_searcher_assign_top(fake, _ffi.f32p(lab), 2, 8, float("inf"), None, 0, 0, *tail) == PCV_ERR_INVALID  # (a valid bound: the handle)
    assert b"searcher is NULL" in L.pcv_last_error()
    assert L.pcv_searcher_last_assign_top_stats(fake, None) == PCV_ERR_INVALID
    assert L.pcv_searcher_last_assign_top_stats(None, C.byref(_ffi.AssignTopStats())) == PCV_ERR_INVALID
    assert n.value == -5  # nothing was written


def test_stats_mirror_matches_the_header():
    names = [f for f, _ in _ffi.AssignTopStats._fields_]
    assert names == ["rows", "candidates", "listed", "m", "label_tiles", "tile_labels", "reruns", "prep_ms", "bound_ms", "screen_ms",
                     "rescore_ms", "select_ms"]
    assert C.sizeof(_ffi.AssignTopStats) == 3 * 8 + 4 * 4 + 5 * 4 + 4  # (padded to the int64 alignment)


@pytest.fixture(scope="module")
def case(golden_dir):
    g = np.load(os.path.join(golden_dir, "scan_n77_d100.npz"))
    rows = np.array(g["corpus"], dtype=np.float32)
    rng = np.random.default_rng(5)
    labels = rng.standard_normal((9, rows.shape[1])).astype(np.float32)
    labels[4] = labels[1]                        # a tie: the lower label first, everywhere
    labels[6] = rows[10] * np.float32(0.5)       # the best of row 10
    rows[20] = 0.0                               # no cosine; a dot product of 0 with every label
    return rows, labels


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("m", [1, 2, 3, 8])
def test_reference_is_the_definition(oracle, case, m, metric):
    rows, labels = case
    K = labels.shape[0]
    for min_score in (None, 0.05):
        want = brute_force(oracle, rows, labels, m, min_score, metric)
        got = assign_top_reference(oracle, rows, labels, m, min_score, metric)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(bits(g) if g.dtype == np.float32 else g, bits(w) if w.dtype == np.float32 else w)
        lab, score, counts, label_rows = got
        assert label_rows.sum() == counts.sum() == (lab >= 0).sum()
        if min_score is None:
            expect = 0 if metric == "cosine" else min(m, K)
            assert counts[20] == expect and (np.delete(counts, 20) == min(m, K)).all()
            assert lab[10, 0] == 6 or metric == "dot"
        else:
            assert counts.max() <= min(m, K) and (counts < min(m, K)).any()
        # a tie: label 4 never comes before label 1, and follows it at once where both are listed
        for r in range(rows.shape[0]):
            listed = list(lab[r, : counts[r]])
            if 4 in listed and r != 20:  # (under dot the zero row ties with every label: all in label order)
                assert listed.index(1) + 1 == listed.index(4)
    if m == 1:
        a_lab, a_score, a_counts = assign_reference(oracle, rows, labels, metric)
        lab, score, counts, label_rows = assign_top_reference(oracle, rows, labels, 1, None, metric)
        np.testing.assert_array_equal(lab[:, 0], a_lab)
        np.testing.assert_array_equal(bits(score[:, 0]), bits(a_score))
        np.testing.assert_array_equal(label_rows, a_counts)
        np.testing.assert_array_equal(counts, (a_lab >= 0).astype(np.int32))
