"""CPU: the magnitude cases of tests/magnitude_ref.py against the oracle — the power-of-two invariance the GPU tests rest on, the
class (inside / outside the f32 envelope of the kernels) every builder claims, and the searchability of the edge rows."""
import numpy as np
import pytest

import magnitude_ref as mr

DIMS = [96, 384, 1024]
K = 300


def topk(oracle, q, rows, metric, k=K):
    return oracle.topk(q, rows, k, metric=1 if metric == "dot" else 0)


@pytest.fixture(scope="module")
def plain(oracle):
    """oracle.topk of the first 8 base queries over the base rows, once per (D, metric)"""
    out = {}
    for D in DIMS:
        rows, queries = mr.base(D)
        for metric in ("cosine", "dot"):
            out[D, metric] = topk(oracle, queries[:8], rows, metric)
    return out


@pytest.mark.parametrize("D", DIMS)
def test_cosine_is_invariant_bit_for_bit(oracle, plain, D):
    rows, queries, er, eq = mr.cosine_wide(D)
    assert er.min() == mr.WIDE_ROW_EXP[0] and er.max() == mr.WIDE_ROW_EXP[1]
    full = er[:er.size // 32 * 32].reshape(-1, 32)
    assert (full.max(1) - full.min(1) == er.max() - er.min()).all()  # every block spans the range
    pos0, sc0, cnt0 = plain[D, "cosine"]
    for r, q in ((rows, queries[:8]), (mr.base(D)[0], queries[:8]), (rows, mr.base(D)[1][:8])):
        pos, sc, cnt = topk(oracle, q, r, "cosine")
        np.testing.assert_array_equal(pos, pos0)
        np.testing.assert_array_equal(sc.view(np.uint64), sc0.view(np.uint64))
        np.testing.assert_array_equal(cnt, cnt0)
    # rows moved to their second exponents (the GPU test's update_items) are the same rows again
    pos, sc, _ = topk(oracle, queries[:8], mr.scaled_rows(D, mr.other_exponents(D)), "cosine")
    np.testing.assert_array_equal(pos, pos0)
    np.testing.assert_array_equal(sc.view(np.uint64), sc0.view(np.uint64))
    assert (mr.other_exponents(D) != er).all()


@pytest.mark.parametrize("ab", mr.DOT_UNIFORM)
@pytest.mark.parametrize("D", DIMS)
def test_dot_scales_by_the_exact_power(oracle, plain, D, ab):
    a, b = ab
    rows, queries = mr.dot_uniform(D, a, b)
    pos0, sc0, cnt0 = plain[D, "dot"]
    pos, sc, cnt = topk(oracle, queries[:8], rows, "dot")
    np.testing.assert_array_equal(pos, pos0)
    np.testing.assert_array_equal(sc, np.ldexp(sc0, a + b))
    np.testing.assert_array_equal(cnt, cnt0)


@pytest.mark.parametrize("D", DIMS)
def test_dot_mixed_moves_only_the_scaled_rows(oracle, D):
    rows, queries = mr.dot_mixed(D)
    base_rows = mr.base(D)[0]
    for q in queries[:4]:
        c = np.array([oracle.canonical_score(q, x, 1) for x in rows[mr.MIXED_SMALL_BLOCK * 32 - 2:mr.MIXED_SMALL_BLOCK * 32 + 34]])
        c0 = np.array([oracle.canonical_score(q, x, 1) for x in base_rows[mr.MIXED_SMALL_BLOCK * 32 - 2:mr.MIXED_SMALL_BLOCK * 32 + 34]])
        np.testing.assert_array_equal(c[:2], c0[:2])
        np.testing.assert_array_equal(c[2:34], np.ldexp(c0[2:34], -40))
        np.testing.assert_array_equal(c[34:], c0[34:])
        assert oracle.canonical_score(q, rows[mr.MIXED_BIG_ROW], 1) == np.ldexp(oracle.canonical_score(q, base_rows[mr.MIXED_BIG_ROW], 1), 40)


# ---- the class every builder claims --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_inside_cases_are_inside(D):
    rows, queries, _, _ = mr.cosine_wide(D)
    for r, q, metric in [(rows, queries, "cosine"), (mr.scaled_rows(D, mr.other_exponents(D)), queries, "cosine"),
                         (mr.dot_mixed(D)[0], mr.dot_mixed(D)[1], "dot")]:
        env = mr.envelope(r, q, metric, D)
        assert env["inside"], env["outside"]
    # 96 features: |q||x| of the (-60, -60) case is 96 * 2^-120 and margin32 = 2 eps32 |q||x| ~ 2^-128 a subnormal; the GPU tests run
    # the dot cases at 384 features, where every case is inside
    for a, b in mr.DOT_UNIFORM:
        env = mr.envelope(*mr.dot_uniform(D, a, b), "dot", D)
        assert env["outside"] == (["margin32"] if (D, a, b) == (96, -60, -60) else []), (a, b, env["outside"])


@pytest.mark.parametrize("D", [384, 1024])
def test_edge_case_leaves_through_the_scales_alone(D):
    e = mr.cosine_edge(D)
    env = mr.envelope(e.rows, e.queries, "cosine", D)
    # the large rows have a subnormal scale, the |q| = 2^127 query a subnormal 1 / |q|, and q'.x over an unscaled row of norm
    # >= 2^128 can pass FLT_MAX; the quantisation scales and margins (formed from y = x * scale, |y| <= 1) stay inside
    assert env["outside"] == ["accumulator", "inv_q", "row_scale"]


@pytest.mark.parametrize("name", mr.DOT_OUTSIDE)
def test_outside_cases_leave_where_they_claim(oracle, name):
    rows, queries, claimed = mr.dot_outside(384, name)
    env = mr.envelope(rows, queries, "dot", 384)
    assert env["outside"] == sorted(claimed)
    assert np.isfinite(rows).all() and np.isfinite(queries).all()
    # the oracle still scores every pair: the contract (finite squared norm) holds
    pos, sc, cnt = topk(oracle, queries[:2], rows, "dot", 10)
    assert (cnt == 10).all() and np.isfinite(sc).all()


# ---- edge rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [384, 1024])
def test_edge_rows_are_searchable_as_the_oracle_says(oracle, D):
    e = mr.cosine_edge(D)
    scale, nx = mr.row_scale(e.rows, "cosine")
    q = mr.base(D)[1][3]
    for name, p in e.pos.items():
        c = oracle.canonical_score(q, e.rows[p], 0)
        assert np.isnan(c) != e.searchable[name], (name, c)
        assert (scale[p] != 0) == e.searchable[name], name
    assert nx[e.pos["norm_at_boundary"]] == 2.0 ** -126
    assert nx[e.pos["norm_below_boundary"]] < 2.0 ** -126 < nx[e.pos["norm_above_subnormal_rest"]]
    # the queries on both sides of nq = 2^-126
    x = mr.base(D)[0][0]
    for i, live in enumerate(e.live):
        assert np.isnan(oracle.canonical_score(e.queries[i], x, 0)) != live, i
    # near copies rank their row first; the near-rank queries put it at the edge of a top-10 list
    for name in e.LARGE:
        pos, _, _ = oracle.topk(e.queries[e.near_copy[name]][None, :], e.rows, 1)
        assert pos[0, 0] == e.pos[name]
    assert set(e.near_rank_queries(oracle, 10)) == set(e.LARGE)


@pytest.mark.parametrize("D", [384, 1024])
def test_large_rows_have_a_subnormal_scale(D):
    """The scale of a row with |x| > 2^126 keeps 23 - (log2|x| - 126) bits.  Printed: its relative error against float64 beside the
    int8 / 6-bit tests' allowance "2e-6 relative" (scan_kernels.hip: T'_q lowered by 2e-6) and beside margin32 = 2 eps32, the f32
    screens' allowance — which of the two a GPU case with such a row stresses."""
    e = mr.cosine_edge(D)
    env = mr.envelope(e.rows, e.queries, "cosine", D)
    scale, nx = env["row_scale"]["value"], mr.row_scale(e.rows, "cosine")[1]
    m32 = float(env["margin32"]["value"][0])
    for name in e.LARGE:
        p = e.pos[name]
        assert 0 < scale[p] < mr.F32_TINY, name
        exact = 1.0 / np.sqrt(nx[p])
        rel = abs(float(scale[p]) - exact) / exact
        half_ulp = 2.0 ** -150 / exact  # a subnormal is a multiple of 2^-149
        assert rel <= half_ulp
        print(f"D={D} {name}: |x| = 2^{0.5 * np.log2(nx[p]):.2f}, scale {float(scale[p]):.6e}, relative error {rel:.3e} "
              f"(half an ulp: {half_ulp:.3e}); int8 / 6-bit allowance 2e-6, margin32 {m32:.3e}")
