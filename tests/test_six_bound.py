"""The 6-bit screen's certificate (csrc/scan.h), checked in numpy against exact scores: for every (row, query),
|c - (4 acc - 126.5 sum q^) / (s_blk s_q)| <= |q'|_2 r_blk + |e_q|_2 n_blk, on rows chosen to quantise badly."""
import numpy as np


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
