"""CPU: item labels (pcv_searcher_assign, _label_sums, _kmeans) without a device — the argument errors that come back before any
device work, and the references the GPU tests compare with (assign_ref.py) against the definition itself."""
import ctypes as C
import os

import numpy as np

from assign_ref import assign_reference, brute_force, bits, sums_reference, unit_ints
from perceive_amd import _ffi

PCV_ERR_INVALID = 1


def test_argument_errors_without_a_device():
    L = _ffi.lib()
    lab = np.zeros((2, 8), dtype=np.float32)
    out = np.zeros(4, dtype=np.int32)
    n = C.c_int64(-5)
    fake = C.c_void_p(0)  # no searcher: every check below comes before the handle is looked at
    assert L.pcv_searcher_assign(fake, None, 2, None, 0, 0, None, None, None, None, C.byref(n)) == PCV_ERR_INVALID
    assert b"NULL" in L.pcv_last_error()
    assert L.pcv_searcher_assign(fake, _ffi.f32p(lab), 2, None, 0, 0, None, None, None, None, None) == PCV_ERR_INVALID
    for k in (0, -1, 4097):
        assert L.pcv_searcher_assign(fake, _ffi.f32p(lab), k, None, 0, 0, None, None, None, None, C.byref(n)) == PCV_ERR_INVALID
        assert b"outside [1,4096]" in L.pcv_last_error()
    assert L.pcv_searcher_assign(fake, _ffi.f32p(lab), 2, None, 0, 4, None, None, None, None, C.byref(n)) == PCV_ERR_INVALID  # no out_label
    assert L.pcv_searcher_assign(fake, _ffi.f32p(lab), 2, None, 0, 4, _ffi.i32p(out), None, None, None, C.byref(n)) == PCV_ERR_INVALID
    assert b"searcher is NULL" in L.pcv_last_error()
    cent = np.zeros((2, 8), dtype=np.float32)
    args = (None, 0, 4, _ffi.f32p(cent), _ffi.i32p(out), None, None, None, None, None, C.byref(n))
    assert L.pcv_searcher_kmeans(fake, None, 2, 3, *args) == PCV_ERR_INVALID
    assert L.pcv_searcher_kmeans(fake, _ffi.f32p(lab), 0, 3, *args) == PCV_ERR_INVALID
    assert L.pcv_searcher_kmeans(fake, _ffi.f32p(lab), 2, -1, *args) == PCV_ERR_INVALID
    assert b"negative" in L.pcv_last_error()
    assert L.pcv_searcher_kmeans(fake, _ffi.f32p(lab), 2, 3, None, 0, 4, None, _ffi.i32p(out), None, None, None, None, None, C.byref(n)) == PCV_ERR_INVALID
    assert L.pcv_searcher_kmeans(fake, _ffi.f32p(lab), 2, 3, *args) == PCV_ERR_INVALID
    assert b"searcher is NULL" in L.pcv_last_error()
    sums = np.zeros((2, 8), dtype=np.int64)
    assert L.pcv_searcher_label_sums(fake, None, 0, _ffi.i32p(out), 4, 2, None, None) == PCV_ERR_INVALID
    assert L.pcv_searcher_label_sums(fake, None, 0, _ffi.i32p(out), 4, 5000, _ffi.i64p(sums), None) == PCV_ERR_INVALID
    assert L.pcv_searcher_label_sums(fake, None, 0, _ffi.i32p(out), 4, 2, _ffi.i64p(sums), None) == PCV_ERR_INVALID
    assert L.pcv_searcher_last_assign_stats(fake, None) == PCV_ERR_INVALID
    assert n.value == -5  # nothing was written


def test_reference_is_the_definition(oracle, golden_dir):
    g = np.load(os.path.join(golden_dir, "scan_n77_d100.npz"))
    rows = np.array(g["corpus"], dtype=np.float32)
    rng = np.random.default_rng(5)
    labels = rng.standard_normal((9, rows.shape[1])).astype(np.float32)
    labels[4] = labels[1]                        # a tie: the lower label everywhere
    labels[6] = rows[10] * np.float32(0.5)       # the best of row 10
    rows[20] = 0.0                               # no cosine; a dot product of 0 with every label
    for metric in ("cosine", "dot"):
        lab, score, counts = assign_reference(oracle, rows, labels, metric)
        b_lab, b_score = brute_force(oracle, rows, labels, metric)
        np.testing.assert_array_equal(lab, b_lab)
        np.testing.assert_array_equal(bits(score), bits(b_score))
        assert (lab != 4).all() and lab[10] == 6 and counts.sum() == (lab >= 0).sum()
        assert (lab[20] == -1 and np.isnan(score[20])) if metric == "cosine" else (lab[20] == 0 and score[20] == 1.0)


def test_integer_sums_do_not_depend_on_the_order():
    rng = np.random.default_rng(6)
    rows = (rng.standard_normal((500, 96)) * rng.uniform(1e-3, 1e3, size=(500, 1))).astype(np.float32)
    rows[7] = 0.0
    lab = rng.integers(-1, 5, size=500)
    t, has = unit_ints(rows)
    assert np.abs(t).max() <= 2 ** 32 and not has[7]
    S, members = sums_reference(rows, lab, 5)
    order = rng.permutation(500)
    S2, members2 = sums_reference(rows[order], lab[order], 5)
    np.testing.assert_array_equal(S, S2)
    np.testing.assert_array_equal(members, members2)
    # ... nor on the shape of the reduction tree: halves summed apart
    half = 250
    Sa, _ = sums_reference(rows[:half], lab[:half], 5)
    Sb, _ = sums_reference(rows[half:], lab[half:], 5)
    np.testing.assert_array_equal(S, Sa + Sb)
    assert members.sum() == ((lab >= 0) & has).sum()
