"""GPU: search and row jobs across the magnitude range (tests/magnitude_ref.py, DESIGN.md "Magnitudes").

Inside the f32 envelope of the kernels a row or query times a power of two changes no canonical cosine and no bit of y = x * scale,
so searcher B, built on the scaled rows, must return what searcher A, built on the plain rows, returns — ids, f32 score bits and,
in a range pass (fixed thresholds), the number of rows through every screen — and A is held to the oracle in the same test.  The
edge rows (norm at 2^-126, subnormal features, subnormal row scales) and the dot cases are held to the oracle alone."""
import numpy as np
import pytest

import magnitude_ref as mr
import neighbors_ref
import perceive_amd as pa
from assign_ref import assign_reference, check_assign
from duplicates_ref import check as check_duplicates
from duplicates_ref import reference as duplicates_reference
from perceive_amd import _ffi
from test_range_gpu import Ranking, check
from test_repack_gpu import reported

pytestmark = pytest.mark.gpu

ATOL = 1e-7  # one f32 ulp of a cosine (test_pass_gpu.py)
FORCE_SIX, FOUR_WAVE, TILE128, VALU_SEED, SEED16, NO_GUESS = 0x80000000, 0x10000000, 8, 4, 2, 32
WAVE, MFMA = _ffi.KERNEL_WAVE, _ffi.KERNEL_MFMA

# name -> (set_kernel, set_screening_copy, set_mid_copy, tuning word, query counts, (kernel_used, screening_copy, screen_bits, mid_copy))
FORMS = {
    "wave": ("wave", "off", "off", 0, (1, 4), (WAVE, 0, 0, 0)),
    "mfma_f32": ("mfma", "off", "off", 0, (8,), (MFMA, 0, 0, 0)),
    "bf16": ("mfma", "bf16", "off", 0, (8, 64), (MFMA, 1, 0, 0)),
    "int8_drain": ("auto", "int8", "off", 0, (8, 33, 64), (MFMA, 2, 8, 0)),  # one tile of 32 queries, then two
    "int8_hold": ("auto", "int8", "off", 0, (100,), (MFMA, 2, 8, 0)),        # the block-holding form
    "int8_tile128": ("auto", "int8", "off", TILE128, (100,), (MFMA, 2, 8, 0)),
    "int8_four_wave": ("auto", "int8", "off", FOUR_WAVE, (16, 64), (MFMA, 2, 8, 0)),
    "int8_mid": ("auto", "int8", "on", 0, (8, 64), (MFMA, 2, 8, 1)),
    "six": ("auto", "auto", "off", FORCE_SIX, (8, 64), (MFMA, 2, 6, 0)),
    "valu_seed": ("auto", "int8", "off", VALU_SEED, (8,), (MFMA, 2, 8, 0)),
    "seed16": ("auto", "int8", "off", SEED16 | VALU_SEED, (8,), (MFMA, 2, 8, 0)),
    "no_guess": ("auto", "int8", "off", NO_GUESS, (8,), (MFMA, 2, 8, 0)),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_ids(n):
    return (np.random.default_rng(5).permutation(n) * 7 + 1000).astype(np.int64)


def build(ctx, rows, ids, metric, form):
    kernel, copy, mid, tuning = FORMS[form][:4]
    s = pa.Searcher(ctx, rows.shape[1], metric)
    s.set_kernel(kernel)
    s.set_tuning(tuning)
    s.set_screening_copy(copy)
    s.set_mid_copy(mid)
    # source 1 in two add_rows rounds, then source 2: segment boundaries inside the scaled data, neither on a block boundary
    c1, c2 = rows.shape[0] // 3, 2 * rows.shape[0] // 3
    s.add_rows(1, rows[:c1], ids[:c1])
    s.finalize()
    s.add_rows(1, rows[c1:c2], ids[c1:c2])
    s.add_rows(2, rows[c2:], ids[c2:])
    s.finalize()
    assert s.num_rows == rows.shape[0] and s.num_segments >= 2
    return s


# (last_stats has nothing finer than these four: the block-holding, tile128, four-wave, VALU-seed, seed16 and no-guess forms all
# report (MFMA, 2, 8, 0), so for them the tuning word and the query count are trusted to select the form, as tests/screens_ref.py
# lays out; what is confirmed is the kernel family, the copy streamed, its width and the mid copy)
def ran_as(s, form):
    st = s.last_stats()
    assert (st["kernel_used"], st["screening_copy"], st["screen_bits"], st["mid_copy"]) == FORMS[form][5], (form, st)
    return st


def same_bits(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]))
    np.testing.assert_array_equal(got[2], want[2])


# ---- (a) cosine, wide --------------------------------------------------------------------------------------------------------------
_wide = {}


def wide_case(oracle, D):
    """plain and scaled rows and queries, ids, the oracle's top 300 and full ranking for 128 plain queries, and the range bounds"""
    if D not in _wide:
        rows_a = mr.base(D)[0]
        rows_b = mr.cosine_wide(D)[0]
        q_plain, q_scaled = mr.wide_queries(D, 128)
        ids = make_ids(rows_a.shape[0])
        opos, osc, ocnt = oracle.topk(q_plain, rows_a, 300)
        assert (ocnt == 300).all()
        rank = Ranking(oracle, q_plain, rows_a, ids, "cosine")
        bounds = osc[:, 59].astype(np.float32)
        _wide[D] = (rows_a, rows_b, q_plain, q_scaled, ids, opos, osc, rank, bounds)
    return _wide[D]


def compare_wide(a, b, case, form):
    rows_a, rows_b, q_plain, q_scaled, ids, opos, osc, rank, bounds = case
    for B in FORMS[form][4]:
        for k in (10, 300):
            got_a = a.search_vectors(None, k, q_plain[:B])
            ran_as(a, form)
            # A against the oracle
            np.testing.assert_array_equal(got_a[0], ids[opos[:B, :k]])
            np.testing.assert_allclose(got_a[1], osc[:B, :k].astype(np.float32), rtol=0, atol=ATOL)
            assert (got_a[2] == k).all()
            # B against A, and scaled queries on both
            same_bits(b.search_vectors(None, k, q_plain[:B]), got_a)
            ran_as(b, form)
            same_bits(a.search_vectors(None, k, q_scaled[:B]), got_a)
            same_bits(b.search_vectors(None, k, q_scaled[:B]), got_a)
    B = max(FORMS[form][4])
    got_a = a.search_range(None, bounds[:B], q_plain[:B], 256)
    st_a = ran_as(a, form)
    got_b = b.search_range(None, bounds[:B], q_scaled[:B], 256)
    st_b = ran_as(b, form)
    for q in range(B):
        wi, ws = rank.expect(q, bounds[q])
        assert 20 <= len(wi) < 200
        check(got_a, wi, ws, q, 256)
        n = int(got_a[2][q])
        np.testing.assert_array_equal(got_b[0][q, :n], got_a[0][q, :n])
        np.testing.assert_array_equal(bits(got_b[1][q, :n]), bits(got_a[1][q, :n]))
    np.testing.assert_array_equal(got_b[2], got_a[2])
    np.testing.assert_array_equal(got_b[3], got_a[3])
    print(f"{form} B={B}: coarse {st_a['coarse_survivors']} / {st_b['coarse_survivors']}, mid {st_a['mid_survivors']} / "
          f"{st_b['mid_survivors']}, narrow {st_a['narrow_survivors']} / {st_b['narrow_survivors']}")
    # the copies are the same bits, so the same rows pass every screen of a pass with fixed thresholds
    for key in ("coarse_survivors", "mid_survivors", "narrow_survivors"):
        assert st_b[key] == st_a[key], key


def run_wide(ctx, oracle, form, D):
    case = wide_case(oracle, D)
    rows_a, rows_b, ids = case[0], case[1], case[4]
    a, b = build(ctx, rows_a, ids, "cosine", form), build(ctx, rows_b, ids, "cosine", form)
    try:
        compare_wide(a, b, case, form)
        # half of B's rows move to another exponent, and are hidden and shown again: the updated and repacked copies are A's still
        moved = np.arange(0, rows_a.shape[0], 2)
        found, n_changed = b.update_items(ids[moved], mr.scaled_rows(D, mr.other_exponents(D))[moved])
        assert found.all() and n_changed == moved.size
        assert b.hide_items(ids[moved]) == moved.size
        hid = b.search_vectors(None, 10, case[2][:1])
        assert not np.isin(hid[0], ids[moved]).any()
        assert b.unhide_items(ids[moved]) == moved.size and b.hidden_rows == 0
        compare_wide(a, b, case, form)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_cosine_wide_scaled_rows_are_the_same_rows(ctx, oracle, form):
    run_wide(ctx, oracle, form, 384)


@pytest.mark.parametrize("form,D", [("int8_drain", 96), ("six", 96), ("bf16", 96), ("int8_drain", 1024), ("int8_mid", 1024), ("wave", 1024)])
def test_cosine_wide_at_other_widths(ctx, oracle, form, D):
    """96 features (padded to 128) and 1024, where a row scaled by 2^120 has a scale just above the smallest normal f32"""
    run_wide(ctx, oracle, form, D)


# ---- (b) cosine, edge ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,D", [("int8_drain", 384), ("int8_mid", 384), ("six", 384), ("bf16", 384), ("wave", 384), ("mfma_f32", 384),
                                    ("int8_drain", 1024), ("int8_mid", 1024), ("bf16", 1024), ("wave", 1024)])  # (no 6-bit copy above 384-d)
def test_cosine_edge_rows(ctx, oracle, form, D):
    """wave, mfma_f32 (fine_survivors) and the int8 forms (drain wave) are the three places an f32 accumulator runs over an unscaled
    row (screen_score): each loses the rows of norm >= 2^128 at k = the number of rows without it"""
    e = mr.cosine_edge(D)
    near = e.near_rank_queries(oracle, 10)
    queries = np.concatenate([e.queries, np.stack([near[name] for name in e.LARGE])])
    live = np.array(e.live + [True] * len(e.LARGE))
    n = e.rows.shape[0]
    ids = make_ids(n)
    unsearchable = [ids[e.pos[name]] for name, ok in e.searchable.items() if not ok]
    s = build(ctx, e.rows, ids, "cosine", form)
    try:
        for k in (10, n):
            opos, osc, ocnt = oracle.topk(queries, e.rows, k)
            got = s.search_vectors(None, k, queries)
            ran_as(s, form)
            np.testing.assert_array_equal(got[2], ocnt)
            assert (got[2][~live] == 0).all() and (got[2][live] == min(k, n - len(unsearchable))).all()
            want_ids = np.where(opos >= 0, ids[np.maximum(opos, 0)], -1)
            np.testing.assert_array_equal(got[0], want_ids)
            for q in range(len(queries)):
                c = int(ocnt[q])
                np.testing.assert_allclose(got[1][q, :c], osc[q, :c].astype(np.float32), rtol=0, atol=ATOL)
            assert not np.isin(got[0], unsearchable).any()
        # a near copy of a large row ranks it first (the near-rank queries are held by the id comparison above)
        got = s.search_vectors(None, 10, queries)
        for name in e.LARGE:
            assert got[0][e.near_copy[name], 0] == ids[e.pos[name]], name
    finally:
        s.close()


# ---- (c) dot, uniform and mixed ------------------------------------------------------------------------------------------------------
DOT_FORMS = ["wave", "mfma_f32", "bf16", "int8_drain", "int8_hold", "int8_tile128", "int8_four_wave", "int8_mid", "six", "valu_seed", "seed16",
             "no_guess"]


def one_ulp(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert np.isfinite(got).all()
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.maximum(np.abs(got), np.abs(want))).astype(np.float64)).all()


def run_dot(ctx, oracle, rows, queries, label, forms=DOT_FORMS, ks=(10, 300)):
    D = rows.shape[1]
    ids = make_ids(rows.shape[0])
    q128 = np.concatenate([queries, np.roll(queries, 1, axis=1)])
    opos, osc, ocnt = oracle.topk(q128, rows, max(ks), metric=1)
    assert (ocnt == max(ks)).all()
    want_d = reported(osc, "dot", D)
    searchers = {}
    try:
        for form in forms:
            kernel, copy, mid, tuning, Bs, _ = FORMS[form]
            key = (copy, mid)
            if key not in searchers:
                searchers[key] = build(ctx, rows, ids, "dot", form)
            s = searchers[key]
            s.set_kernel(kernel)
            s.set_tuning(tuning)
            for B in Bs:
                for k in ks:
                    got = s.search_vectors(None, k, q128[:B])
                    st = ran_as(s, form)
                    np.testing.assert_array_equal(got[0], ids[opos[:B, :k]])
                    one_ulp(got[1], want_d[:B, :k])
                    assert (got[2] == k).all()
                    print(f"{label} {form} B={B} k={k}: scan_launches {st['scan_launches']}, overflow_reruns {st['overflow_reruns']}, "
                          f"speculation_reruns {st['speculation_reruns']}, candidates {st['candidates']}")
    finally:
        for s in searchers.values():
            s.close()


@pytest.mark.parametrize("ab", mr.DOT_UNIFORM)
def test_dot_uniform(ctx, oracle, ab):
    rows, queries = mr.dot_uniform(384, *ab)
    run_dot(ctx, oracle, rows, queries, f"uniform{ab}")


def test_dot_mixed(ctx, oracle):
    """one row times 2^40 raises max_norm, and with it every margin, for the whole corpus; one block sits 2^40 below the rest"""
    rows, queries = mr.dot_mixed(384)
    run_dot(ctx, oracle, rows, queries, "mixed")


@pytest.mark.parametrize("D", [96, 1024])
@pytest.mark.parametrize("case", ["up", "down", "mixed"])
def test_dot_at_other_widths(ctx, oracle, case, D):
    """96 features (padded to 128; |q||x| of the (-60, -60) case is 2^-113 there and margin32 a subnormal: check_dot_envelope's
    argument for the floor) and 1024"""
    rows, queries = mr.dot_mixed(D) if case == "mixed" else mr.dot_uniform(D, *{"up": (40, 40), "down": (-60, -60)}[case])
    run_dot(ctx, oracle, rows, queries, f"{case} D={D}", forms=["wave", "bf16", "int8_drain", "int8_mid"] + (["six"] if D == 96 else []))


# ---- (d) dot, outside the f32 envelope -------------------------------------------------------------------------------------------------
# The rule: a result differs from the oracle's only together with an error status.  Per quantity (perceive_hip.h):
#   s_q, unit / margins / accumulators : PCV_ERR_INVALID from the search call, before anything is queued (check_dot_envelope runs in
#       check_search_args, ahead of plan_search; nothing on the device depends on the query yet)
#   s_blk, mid scale                   : exact — the scales are capped (corpus_kernels.hip, kMaxCopyScale), the block's codes are zeros
# Read before the first run: run_pass repeats a pass at most 7 times (searcher_pass.cpp), a ceiling pass is bounded by k / 128, no
# index is formed from a float anywhere in the scans (quantised codes are clamped integers; list positions come from atomic
# counters checked against cand_cap).  Predicted outcome beside each case.
PCV_ERR_INVALID = 1
OUTSIDE = {
    "q_max_2p-121": ("refused", "s_q"),       # max|q_i| = 2^-121 < 2^-120 (s_q itself still finite; margin32 subnormal)
    "q_max_2p-125": ("refused", "s_q"),       # 127 / 2^-125 = inf
    "q_max_subnormal": ("refused", "s_q"),
    "block_max_2p-122": ("exact", None),      # 127 / 2^-122 = inf before the cap; now s_blk = 2^100, codes 0, mid scale 2^108
    "segment_max_2p-122": ("exact", None),    # a whole segment of such blocks
    "margin_2p129": ("refused", "unit"),      # |q| max_norm = 1.02 FLT_MAX
    "products_overflow": ("refused", "unit"),  # q_i x_i ~ 2^140: |q| max_norm = 2^148
    # rows times 2^118, queries times 2^-20: unit ~ 2^107 accepted; T_q = (tau - e32) s_q ~ 2^129 was +inf, T - |T| 2e-6 NaN and no
    # row of any query passed the int8 / 6-bit test.  Predicted with int8_threshold's cap: T_q = FLT_MAX, U = FLT_MAX - c1 (2^126)
    # finite, rhs = s_blk U ~ 2^15 against integer dot products up to 2^22: a looser screen, the oracle's result
    "threshold_2p129": ("exact", None),
}


@pytest.mark.parametrize("name", mr.DOT_OUTSIDE)
def test_dot_outside_is_exact_or_refused(ctx, oracle, name):
    assert set(OUTSIDE) == set(mr.DOT_OUTSIDE)
    outcome, quantity = OUTSIDE[name]
    rows, queries, _ = mr.dot_outside(384, name)
    if outcome == "exact":
        n = rows.shape[0]
        forms = ["int8_drain", "int8_hold", "int8_tile128", "int8_four_wave", "int8_mid", "six"] if name == "threshold_2p129" else \
            ["wave", "bf16", "int8_drain", "int8_mid", "six"]
        run_dot(ctx, oracle, rows, queries if name == "threshold_2p129" else queries[:32], name, forms=forms,
                ks=(10, 300) if name == "threshold_2p129" else (10, n))
        return
    ids = make_ids(rows.shape[0])
    plain = mr.base(384)[1]
    for form in ("int8_drain", "wave"):
        s = build(ctx, rows, ids, "dot", form)
        try:
            for call in (lambda: s.search_vectors(None, 10, queries[:8]),
                         lambda: s.search_range(None, np.zeros(8, np.float32), queries[:8], 16)):
                with pytest.raises(_ffi.PcvError) as err:
                    call()
                print(f"{name} {form}: {err.value}")
                assert err.value.status == PCV_ERR_INVALID and quantity in str(err.value)
            if name.startswith("q_max"):  # the rows are plain: the searcher answers the queries that are inside, exactly
                opos, osc, _ = oracle.topk(plain[8:16], rows, 10, metric=1)
                got = s.search_vectors(None, 10, plain[8:16])
                np.testing.assert_array_equal(got[0], ids[opos])
                one_ulp(got[1], reported(osc, "dot", 384))
        finally:
            s.close()


def test_dot_queries_on_the_device_are_not_read_on_the_host(ctx, oracle):
    """pcv_searcher_search_device_begin_dq under the dot metric: the queries live in device memory, check_dot_envelope must not
    touch them (kEnvelopeNone), and the pass is the exact one.  The same call with host queries checks what every rank evaluates
    alike: s_q."""
    D, k, B = 384, 10, 8
    rows, queries = mr.base(D)
    ids = make_ids(rows.shape[0])
    opos, osc, _ = oracle.topk(queries[:B], rows, k, metric=1)
    s = build(ctx, rows, ids, "dot", "int8_drain")
    rec = B * k + 1
    d_q, d_out = ctx.alloc(B * D * 4), ctx.alloc(rec * 24)
    try:
        ctx.to_device(d_q, queries[:B])
        for attempt in range(8):
            s.search_device_begin_dq(None, k, d_q, B, d_out)
            over = s.search_device_end()
            got = pa.merge_topk(ctx, "dot", D, d_out, 1, B, k, flagged=True)
            assert got[3] == over
            if not over:
                break
        assert not over
        np.testing.assert_array_equal(got[0], ids[opos])
        one_ulp(got[1], reported(osc, "dot", D))
        tiny = mr.dot_outside(D, "q_max_2p-125")[1][:B]
        with pytest.raises(_ffi.PcvError) as err:
            s.search_device_begin(None, k, tiny, d_out)
        assert err.value.status == PCV_ERR_INVALID and "s_q" in str(err.value)
    finally:
        ctx.free(d_q)
        ctx.free(d_out)
        s.close()


# ---- (e) row jobs that share the row scale -------------------------------------------------------------------------------------------
NO_COSINE = (41, 76, 500, 2999)  # a norm one ulp below 2^-63, subnormal features only, all zero, a feature that is inf
N_COPIES = 20


def row_job_case():
    D = 96
    rng = np.random.default_rng(31)
    rows_a = mr.base(D)[0].copy()
    src = rng.choice(np.arange(100, 2900), N_COPIES, replace=False)
    dst = np.setdiff1d(np.arange(100, 2900), np.concatenate([src, NO_COSINE]))[:: 2800 // N_COPIES - 1][:N_COPIES]
    rows_a[dst] = rows_a[src]  # B holds them at other exponents
    e = mr.cosine_wide(D)[2].copy()
    e[dst] = np.where(e[src] > 0, e[src] - 50, e[src] + 50)
    e[list(NO_COSINE)] = 0
    rows_b = mr.scale_pow2(rows_a, e)
    for r in (rows_a, rows_b):
        r[NO_COSINE[0]] = 0
        r[NO_COSINE[0], 7] = np.nextafter(np.float32(2.0 ** -63), np.float32(0))
        r[NO_COSINE[1]] = np.float32(2.0 ** -140)
        r[NO_COSINE[2]] = 0
        r[NO_COSINE[3], 11] = np.inf
    labels_a = mr.base(D)[1][:16]
    labels_b = mr.cosine_wide(D)[1][:16]
    return rows_a, rows_b, labels_a, labels_b


def test_row_jobs_on_scaled_rows(ctx, oracle):
    rows_a, rows_b, labels_a, labels_b = row_job_case()
    n = rows_a.shape[0]
    ids = make_ids(n)
    part = neighbors_ref.takes_part(rows_b)
    np.testing.assert_array_equal(part, neighbors_ref.takes_part(rows_a))
    assert not part[list(NO_COSINE)].any() and part.sum() == n - len(NO_COSINE)
    a, b = build(ctx, rows_a, ids, "cosine", "int8_drain"), build(ctx, rows_b, ids, "cosine", "int8_drain")
    try:
        # neighbours
        nb_a, nb_b = a.neighbors(None, 8), b.neighbors(None, 8)
        for x, y in zip(nb_a, nb_b):
            np.testing.assert_array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
        neighbors_ref.check(nb_b, neighbors_ref.reference(oracle, rows_b, ids, 8))
        neighbors_ref.check(nb_a, neighbors_ref.reference(oracle, rows_a, ids, 8))
        assert (nb_b[3][list(NO_COSINE)] == 0).all() and not np.isin(nb_b[1], ids[list(NO_COSINE)]).any()
        # labels
        as_a, as_b = a.assign(None, labels_a), b.assign(None, labels_b)
        for x, y in zip(as_a, as_b):
            np.testing.assert_array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
        check_assign(as_b, assign_reference(oracle, rows_b, labels_b, part=part), ids)
        check_assign(as_a, assign_reference(oracle, rows_a, labels_a, part=part), ids)
        assert (as_b[0][list(NO_COSINE)] == -1).all() and np.isnan(as_b[1][list(NO_COSINE)]).all()
        # duplicate pairs: Gaussian rows of 96 features stay below cosine 0.6 of each other; the planted copies are at 1
        du_a, du_b = a.find_duplicates(None, 0.9), b.find_duplicates(None, 0.9)
        assert du_a[3] == du_b[3] == N_COPIES
        for x, y in zip(du_a[:3], du_b[:3]):
            np.testing.assert_array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
        check_duplicates(du_b, duplicates_reference(oracle, rows_b, ids, 0.9, part=np.flatnonzero(part)))
        check_duplicates(du_a, duplicates_reference(oracle, rows_a, ids, 0.9, part=np.flatnonzero(part)))
        assert not np.isin(np.concatenate([du_b[0], du_b[1]]), ids[list(NO_COSINE)]).any()
    finally:
        a.close()
        b.close()
