"""The 6-bit screen's certificate (csrc/scan.h), checked in numpy against exact scores: for every (row, query),
|c - (4 acc - 126.5 sum q^) / (s_blk s_q)| <= |q'|_2 r_blk + |e_q|_2 n_blk, on rows chosen to quantise badly."""
import numpy as np
import pytest

import six_ref


def quantise_blocks(y):
    """int8 copy as coarse_pack8_kernel makes it (one scale per 32-row block), then the 6-bit codes and the block constants."""
    n, D = y.shape
    x8 = np.zeros_like(y, dtype=np.int32)
    s = np.zeros(n)
    for b in range(0, n, 32):
        blk = y[b : b + 32]
        m = np.abs(blk).max()
        sb = 127.0 / m if m > 0 else 1.0
        x8[b : b + 32] = np.clip(np.rint(blk.astype(np.float32) * np.float32(sb)), -127, 127)
        s[b : b + 32] = np.float32(sb)
    h = x8 >> 2
    xt = (4.0 * h + 1.5) / s[:, None]
    r = np.linalg.norm(y - xt, axis=1)
    nn = np.linalg.norm(xt, axis=1)
    rb = np.repeat([r[b : b + 32].max() for b in range(0, n, 32)], 32)[:n]
    nb = np.repeat([nn[b : b + 32].max() for b in range(0, n, 32)], 32)[:n]
    return h + 32, s, rb, nb


def quantise_query(q):
    sq = 127.0 / np.abs(q).max()
    qh = np.clip(np.rint(q * sq), -127, 127)
    return qh, sq, np.linalg.norm(q), np.linalg.norm(q - qh / sq)


def test_l2_bound_holds_on_adversarial_rows():
    rng = np.random.default_rng(0)
    D = 384
    rows = [
        rng.standard_cauchy((256, D)),                                   # one feature dominates each row
        np.eye(D)[rng.integers(0, D, 128)] * rng.standard_normal((128, 1)),  # one-hot rows
        np.full((64, D), 0.37) + 1e-7 * rng.standard_normal((64, D)),    # every value on the same step
        rng.standard_normal((512, D)),
        rng.uniform(-1, 1, (128, D)) ** 9,                               # most values far below the block's largest
    ]
    y = np.concatenate(rows).astype(np.float32)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    y = y[rng.permutation(len(y))].astype(np.float64)
    u, s, rb, nb = quantise_blocks(y)
    queries = np.concatenate([rng.standard_normal((6, D)), rng.standard_cauchy((4, D)), y[:6], np.eye(D)[:2]])
    queries /= np.linalg.norm(queries, axis=1, keepdims=True)
    worst = 0.0
    for q in queries:
        qh, sq, n2, e2 = quantise_query(q)
        acc = u @ qh                                              # exact integers
        est = (4.0 * acc - 126.5 * qh.sum()) / (s * sq)
        c = y @ q
        bound = n2 * rb + e2 * nb
        assert (np.abs(c - est) <= bound * (1 + 1e-9) + 1e-12).all()
        worst = max(worst, (np.abs(c - est) / bound).max())
    assert worst > 0.05  # the rows do come near it


def test_six_bit_codes_stand_for_the_int8_codes():
    # u = (x^ >> 2) + 32 in [0, 63] stands for 4 (u - 32) + 1.5, within 1.5 of x^ (int8 units)
    x8 = np.arange(-127, 128)
    u = (((x8 + 128) & 0xFF) >> 2)
    assert u.min() == 0 and u.max() == 63
    np.testing.assert_array_equal(u, (x8 >> 2) + 32)
    assert np.abs(4 * (u - 32) + 1.5 - x8).max() <= 1.5


# ---- the model of tests/six_ref.py: the certificate at every width, and the bracket the GPU test of the screen's counts rests on ----
WIDTHS = [64, 100, 128, 136, 200, 256, 260, 384]  # padded to 64 / 128 features or not, one to three chunks of 128


def adversarial_rows(rng, D, metric):
    """the row families of test_l2_bound_holds_on_adversarial_rows at width D, 34 blocks, shuffled; dot: norms over three decades"""
    rows = [
        rng.standard_cauchy((256, D)),
        np.eye(D)[rng.integers(0, D, 128)] * rng.standard_normal((128, 1)),
        np.full((64, D), 0.37) + 1e-7 * rng.standard_normal((64, D)),
        rng.standard_normal((512, D)),
        rng.uniform(-1, 1, (128, D)) ** 9,
    ]
    y = np.concatenate(rows)
    y = y[rng.permutation(len(y))]
    if metric == "dot":
        y = y / np.linalg.norm(y, axis=1, keepdims=True) * 10.0 ** rng.uniform(-1.5, 1.5, (len(y), 1))
    return y.astype(np.float32)


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("D", WIDTHS)
def test_certificate_holds_at_every_width(D, metric):
    rng = np.random.default_rng(100 + D)
    x = adversarial_rows(rng, D, metric)[:-7]  # a partial last block
    n = len(x)
    searchable = rng.random(n) > 0.15          # blocks that mix searchable and hidden rows
    searchable[96:128] = False                 # block 3: no searchable row
    x[40] = 0.0                                # cosine: a row without a norm; dot: a searchable all-zero row
    x[192:224] = 0.0                           # block 6 whole: cosine nothing to search, dot s_blk = 1 (if a row of it is searchable)
    searchable[200] = True
    rows = six_ref.Rows(x, metric, searchable)
    assert np.isnan(rows.s_blk[3]) and (rows.codes8[96:128] == 0).all() and (rows.u[96:128] == 32).all()
    assert np.isnan(rows.s_blk[6]) if metric == "cosine" else rows.s_blk[6] == 1.0
    assert not rows.live[n:].any() and rows.live[:n].sum() > 0.7 * n
    assert rows.u.min() >= 0 and rows.u.max() <= 63 and np.abs(rows.codes8).max() == 127
    np.testing.assert_array_equal(rows.u, ((rows.codes8 + 128) & 0xFF) >> 2)
    queries = np.concatenate([rng.standard_normal((6, D)), rng.standard_cauchy((4, D)), x[:6], np.eye(D)[:2], np.zeros((1, D))]).astype(np.float32)
    qs = six_ref.Queries(queries, rows)
    assert qs.s_q[-1] == 0 and (qs.s_q[:-1] > 0).sum() >= 17
    est, bound = six_ref.estimates(rows, qs)
    c = rows.y @ qs.qp.T
    ok = rows.live[:, None] & (qs.s_q != 0)[None, :]
    gap = np.abs(c - est)
    assert (gap[ok] <= bound[ok] * (1 + 1e-9) + 1e-12 * np.maximum(1.0, np.abs(c[ok]))).all()
    assert (gap[ok] / bound[ok]).max() > 0.05  # the rows do come near it
    # the tests built on it lose no row at or above a threshold: tau = each query's 98th percentile over the searchable rows
    alive = qs.s_q != 0
    tau = np.array([np.quantile(c[rows.live, q], 0.98) if alive[q] else 0.0 for q in range(qs.B)])
    six, both = six_ref.keeps(rows, qs, tau)
    above = ok & (c >= tau[None, :])
    assert above.sum() >= 10 * alive.sum()
    assert six[above].all() and both[above].all()
    assert not six[96:128].any() and not both[~six].any()
    # a dead query: cosine keeps nothing, dot every row of a block that has a searchable row
    has_rows = np.repeat(~np.isnan(rows.s_blk), 32)
    np.testing.assert_array_equal(six[:, -1], has_rows if metric == "dot" else np.zeros_like(has_rows))
    # slack: positive loosens, negative tightens, and both nest around the test itself
    s = six_ref.kernel_slack(D)
    lo6, lo8 = six_ref.keeps(rows, qs, tau, -s)
    hi6, hi8 = six_ref.keeps(rows, qs, tau, +s)
    assert (lo6 <= six).all() and (six <= hi6).all() and (lo8 <= both).all() and (both <= hi8).all()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("D", [100, 200, 384])
def test_model_bracket_is_tight(oracle, D, metric):
    """The condition the GPU test of the screen's counts (test_six_paths_gpu.py, fixed thresholds) rests on: over its inputs the
    model's count with both tests tightened by kernel_slack(D) and the count with them loosened by it differ by at most 2 % of
    the looser one — a device count between the two is then within 2 % of the model's.  The slack is derived in
    six_ref.kernel_slack from the roundings the kernels add on purpose; nothing here is tuned against a device."""
    corpus, queries, bounds, in_range, opos, orep = six_ref.range_case(oracle, D, metric)
    rows = six_ref.Rows(corpus, metric)
    qs = six_ref.Queries(queries, rows)
    tau = six_ref.range_tau(bounds, queries, rows)
    s = six_ref.kernel_slack(D)
    lo6, lo8 = six_ref.keeps(rows, qs, tau, -s)
    hi6, hi8 = six_ref.keeps(rows, qs, tau, +s)
    print(f"D={D} {metric}: slack {s:.3e}; 6-bit test keeps {lo6.sum()} .. {hi6.sum()}, both tests {lo8.sum()} .. {hi8.sum()}")
    assert lo6.sum() >= 64 * 20 and lo8.sum() >= 64 * 20
    assert hi6.sum() - lo6.sum() <= 0.02 * hi6.sum()
    assert hi8.sum() - lo8.sum() <= 0.02 * hi8.sum()
    both = six_ref.keeps(rows, qs, tau)[1]
    for q in range(64):  # the tests themselves lose no in-range row
        assert both[opos[q, : in_range[q]], q].all()
