"""A float64 numpy model of the 6-bit screen, written from csrc/scan.h, pack8_block / pack6_kernel (csrc/corpus_kernels.hip) and
quantize_queries_kernel / scan_mfma8_kernel / drain_survivors (csrc/scan_kernels.hip).

Rows.  y = x * scale in f32 (scale = 1/|x| for cosine, 1 for dot, 0 for a row that is not searchable), 32 rows a block, features
padded with zeros to Dp (a multiple of 64; the int8 copy pads on to Dp8, a multiple of 128).  Per block, over its searchable rows:
    s_blk = 127 / max|y_i|  (1 if every searchable row is zero, NaN if the block has no searchable row)
    x^    = clip(rint(y * s_blk), -127, 127)          the int8 codes; zeros for a row that is not searchable
    u     = (x^ >> 2) + 32 in [0, 63]                  the 6-bit codes; u stands for x~ = (4 (u - 32) + 1.5) / s_blk
    r_blk = max |y - x~|_2,  n_blk = max |x~|_2        over the first Dp features: the padding up to Dp counts (y = 0, x~ = 1.5 / s_blk),
                                                       the int8 copy's padding from Dp to Dp8 does not
Queries.  q' = q / |q| (cosine) or q (dot) in f32, s_q = 127 / max|q'_i|, q^ = clip(rint(q' * s_q), -127, 127), e_q = q' - q^ / s_q.

The 6-bit test of (row, query) for a threshold tau on the canonical score, in units of 4 acc (acc = sum u_i q^_i, an exact integer):
    L = 4 acc - 126.5 sum q^ + s_blk s_q (|q'|_2 r_blk + |e_q|_2 n_blk)   >=   s_blk s_q tau = Rhs
and the int8 test of a row that passed it (acc8 = sum x^_i q^_i, the constants are the kernel's own):
    acc8  >=  s_blk (s_q tau - 0.5002 sqrt(Dp8) nrm) - (0.5002 |q'|_1 s_q + 0.2501 Dp8 + 4)        nrm = 1 (cosine), max|x| (dot)
A dead query (s_q = 0: all-zero or without a norm) keeps nothing under cosine and every row of every block that has a searchable
row under dot.  A block without a searchable row keeps nothing (s_blk = NaN).  Every one of a block's 32 rows meets the test, the
ones that are not searchable included (their codes are zeros, u = 32): the kernel sheds them only at the f32 row.

Slack.  Each test takes a relative slack: positive loosens, negative tightens it, by
    |slack| (s_blk s_q unit + |Rhs| + t2) + min(|slack|, WN_SLACK) M          6-bit: t2 = the L2 term, M = 252 sum|q^| + 126.5 |sum q^|
    |slack| (s_blk s_q unit + |s_blk s_q tau| + s_blk c1 + V_q)               int8
unit = the size of a score, 1 (cosine) or |q| max|x| (dot).  kernel_slack(D) is the value that covers what the kernels add to the
test on purpose; its derivation is in its docstring."""
import functools

import numpy as np

WN_SLACK = 2.0 ** -20 + 2.0 ** -21


def padded(D):
    Dp = (D + 63) // 64 * 64
    return Dp, (Dp + 127) // 128 * 128


def eps32(D):
    """the f32 screening score's error bound relative to |q||x| (searcher_pass.cpp, fill_params); margin32 = 2 eps32 unit"""
    return (padded(D)[0] + 16) * 1.2e-7


def kernel_slack(D):
    """What the kernels add to the 6-bit test on purpose, each relative to a quantity the slack multiplies:
      - margin32 / 2 = eps32 unit is taken off tau before anything else, and the dot metric's unit carries a factor 1.0001:
        1.0001 eps32 of s_blk s_q unit;
      - T = (tau - eps32 unit) s_q is lowered by 2e-6 of itself (and rounded twice in f32, 2^-23): 2e-6 + 2^-23 of |Rhs| and of
        s_blk s_q unit;
      - R = s_blk r_blk, N = s_blk n_blk, A = s_q |q'|_2 and E = s_q |e_q|_2 are each raised by 1 + 2^-19 (and rounded to f32 first),
        their sum of products by 1 + 2^-20: (1 + 2^-19)^2 (1 + 2^-20) (1 + 2^-23)^3 - 1 < 2^-18 + 2^-20 + 2^-21 of t2;
      - Wn = -126.5 sum q^ + 2^-20 M, raised by 2^-22 |Wn| <= 2^-22 M, and the f32 roundings of the left-hand side that the 2^-20 M
        is there to cover (four of 2^-24 M at most): 2^-20 + 2^-22 + 2^-22 of M — WN_SLACK, applied to M alone, because M is
        several times the size of a score and eps32 of it would be a far wider band than the kernel's.
    The terms are disjoint, so the largest factor in front of each quantity is enough; the sum of them is taken.  The int8 test
    carries the same tau - eps32 unit and the same 2e-6, and f32 roundings of 2^-24 on each of its terms: less than this."""
    return 1.0001 * eps32(D) + 2e-6 + 2.0 ** -23 + 2.0 ** -18 + 2.0 ** -20 + 2.0 ** -21


def sum_squares(x):
    """|x|^2 per row, f64, accumulated in feature order (row_sum_squares)"""
    nx = np.zeros(x.shape[0])
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(0, x.shape[1], 64):  # (the same additions in the same order, over contiguous columns, 64 at a time)
            for col in np.ascontiguousarray(x[:, j:j + 64].T, dtype=np.float64):
                nx += col ** 2
    return nx


class Rows:
    """The copies of `rows` [n, D] f32 under `metric` ("cosine" | "dot"); `searchable` [n] bool (default: all) marks rows that are
    hidden.  Arrays over rows have nblk * 32 entries: the rows behind n are padding and not searchable."""

    def __init__(self, rows, metric, searchable=None):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n, D = rows.shape
        self.n, self.D, self.metric = n, D, metric
        self.Dp, self.Dp8 = padded(D)
        self.nblk = (n + 31) // 32
        npad = self.nblk * 32
        nx = sum_squares(rows)
        finite = nx < np.inf  # (false for inf and NaN)
        with np.errstate(divide="ignore", invalid="ignore"):
            if metric == "dot":
                scale = np.where(finite, 1.0, 0.0).astype(np.float32)
            else:
                scale = np.where(finite & (nx >= 2.0 ** -126), (1.0 / np.sqrt(nx)), 0.0).astype(np.float32)
        norm32 = np.sqrt(np.where(finite, nx, 0.0)).astype(np.float32) * np.float32(1.000001)
        self.max_norm = float(norm32[scale != 0].max()) if (scale != 0).any() else 0.0  # raise_max_norm: hidden rows count
        if searchable is not None:
            scale = np.where(np.asarray(searchable, dtype=bool), scale, np.float32(0.0)).astype(np.float32)
        self.scale = np.zeros(npad, np.float32)
        self.scale[:n] = scale
        self.nonfinite = np.zeros(npad, bool)  # a row with an inf or a NaN: scale 0, and NaN products where a kernel multiplies anyway
        self.nonfinite[:n] = ~finite
        self.x = np.zeros((npad, self.Dp))     # the f32 rows themselves; zeros for a row without a scale (the fine test ends there)
        self.x[:n, :D] = rows
        self.x[:n][scale == 0] = 0.0
        y = np.zeros((npad, self.Dp), np.float32)
        y[:n, :D] = rows
        with np.errstate(over="ignore", invalid="ignore"):
            y[:n, :D] *= scale[:, None]  # (an f32 product)
        y[:n][scale == 0] = 0.0
        mx = np.maximum(y.max(axis=1), -y.min(axis=1))  # max |y|, NaN where the row has one
        self.live = (self.scale != 0) & (mx < np.inf)
        y[~self.live] = 0.0
        self.y32 = y                           # y as the device has it; `y` is the same in f64, made when it is first read
        liveb = self.live.reshape(self.nblk, 32)
        bm = np.where(liveb, mx.reshape(self.nblk, 32), np.float32(0.0)).max(axis=1).astype(np.float32)
        with np.errstate(divide="ignore"):
            s = np.where(bm > 0, np.float32(127.0) / bm, np.float32(1.0)).astype(np.float32)
        self.s_blk = np.where(liveb.any(axis=1), s, np.float32(np.nan)).astype(np.float32)
        self._s_safe = np.where(liveb.any(axis=1), s, np.float32(1.0)).astype(np.float32)

    # The int8 and 6-bit codes and the 6-bit residual bounds are made when they are first read: a model that never reads them (a
    # screen without such a copy) does not pay for them.
    @functools.cached_property
    def y(self):
        return self.y32.astype(np.float64)

    @functools.cached_property
    def codes8(self):
        yb = self.y32.reshape(self.nblk, 32, self.Dp)
        codes = np.clip(np.rint(yb * self._s_safe[:, None, None]), -127, 127).astype(np.int64)  # (the product is an f32 one)
        codes[~self.live.reshape(self.nblk, 32)] = 0
        return codes.reshape(self.nblk * 32, self.Dp)

    @functools.cached_property
    def u(self):
        return (self.codes8 >> 2) + 32

    @functools.cached_property
    def _six_bounds(self):
        liveb = self.live.reshape(self.nblk, 32)
        inv_s = 1.0 / self._s_safe.astype(np.float64)
        xt = (4.0 * (self.codes8 >> 2).reshape(self.nblk, 32, self.Dp) + 1.5) * inv_s[:, None, None]
        err = np.sqrt(((self.y.reshape(self.nblk, 32, self.Dp) - xt) ** 2).sum(axis=2))
        nrm = np.sqrt((xt ** 2).sum(axis=2))
        return np.where(liveb, err, 0.0).max(axis=1), np.where(liveb, nrm, 0.0).max(axis=1)

    @property
    def r_blk(self):
        return self._six_bounds[0]

    @property
    def n_blk(self):
        return self._six_bounds[1]

    def block_of_rows(self, per_block):
        return np.repeat(per_block, 32)


class Queries:
    """The scan-side form of `queries` [B, D] f32 and the constants of the two tests; `rows` gives the shape, the metric and max|x|."""

    def __init__(self, queries, rows):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        B, D = q.shape
        assert D == rows.D
        self.B = B
        nq = (q.astype(np.float64) ** 2).sum(axis=1)
        if rows.metric == "dot":
            live = nq < np.inf
            inv = np.ones(B, np.float32)
        else:
            live = (nq >= 2.0 ** -126) & (nq < np.inf)
            with np.errstate(divide="ignore"):
                inv = np.where(live, 1.0 / np.sqrt(nq), 0.0).astype(np.float32)
        qp = np.zeros((B, rows.Dp), np.float32)
        qp[:, :D] = np.where(live[:, None], q * inv[:, None], np.float32(0.0))
        self.qp = qp.astype(np.float64)
        mx = np.abs(qp).max(axis=1)
        l1 = np.abs(qp).sum(axis=1, dtype=np.float32)
        ok = (mx > 0) & (mx < np.inf) & (l1 < np.inf)
        with np.errstate(divide="ignore"):
            self.s_q = np.where(ok, np.float32(127.0) / np.where(ok, mx, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        self.qh = np.clip(np.rint(qp * self.s_q[:, None]), -127, 127).astype(np.int64)  # (an f32 product)
        sq64 = self.s_q.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(ok[:, None], self.qp - self.qh / np.where(ok, sq64, 1.0)[:, None], 0.0)
        self.norm2 = np.sqrt((self.qp ** 2).sum(axis=1))   # |q'|_2
        self.err2 = np.sqrt((e ** 2).sum(axis=1))          # |e_q|_2
        self.qsum = self.qh.sum(axis=1)
        self.qabs = np.abs(self.qh).sum(axis=1)
        self.l1 = l1.astype(np.float64)
        self.unit = np.sqrt(nq) * rows.max_norm if rows.metric == "dot" else np.ones(B)


def estimates(rows, qs):
    """the 6-bit estimate (4 acc - 126.5 sum q^) / (s_blk s_q) of y . q' [rows, B] and its certified bound; NaN where either is dead"""
    acc = rows.u @ qs.qh.T
    s = rows.block_of_rows(rows.s_blk.astype(np.float64))[:, None]
    sq = np.where(qs.s_q != 0, qs.s_q, np.nan).astype(np.float64)[None, :]
    est = (4.0 * acc - 126.5 * qs.qsum[None, :]) / (s * sq)
    bound = qs.norm2[None, :] * rows.block_of_rows(rows.r_blk)[:, None] + qs.err2[None, :] * rows.block_of_rows(rows.n_blk)[:, None]
    return est, bound


def _acc8(rows, qs):
    """sum x^_i q^_i [nblk * 32, B], once per (rows, queries): it does not depend on the thresholds"""
    store = rows.__dict__.setdefault("_acc8_memo", {})
    if id(qs) not in store:
        store[id(qs)] = (qs, rows.codes8.astype(np.float64) @ qs.qh.T.astype(np.float64))  # (the queries are held: their id stays theirs)
    return store[id(qs)][1]


def keep_int8(rows, qs, tau, slack=0.0):
    """The int8 test on its own, bool [nblk * 32, B]: acc8 >= s_blk (s_q tau - c1) - V_q with the kernel's constants (the header);
    the slack's quantities are unit, |Rhs|, s_blk c1 and V_q.  The codes are small integers: the float64 product is exact.
    The right-hand side is the same for the 32 rows of a block: it is worked out per block and repeated."""
    tau = np.asarray(tau, dtype=np.float64)
    sgn, a = (1.0 if slack >= 0 else -1.0), abs(slack)
    s = rows.s_blk.astype(np.float64)[:, None]   # [nblk, 1]; NaN: no comparison succeeds
    sq = qs.s_q.astype(np.float64)[None, :]
    with np.errstate(invalid="ignore"):
        ssq = s * sq
        rhs = ssq * tau[None, :]
        nrm = rows.max_norm if rows.metric == "dot" else 1.0
        c1 = 0.5002 * np.sqrt(float(rows.Dp8)) * nrm
        vq = (0.5002 * qs.l1 * qs.s_q + 0.2501 * rows.Dp8 + 4.0)[None, :]
        allow8 = a * (ssq * qs.unit[None, :] + np.abs(rhs) + s * c1 + vq)
        eight = _acc8(rows, qs) >= np.repeat(rhs - s * c1 - vq - sgn * allow8, 32, axis=0)
    dead = (qs.s_q == 0)[None, :]
    if not dead.any():
        return eight
    has_rows = np.repeat(~np.isnan(s), 32, axis=0)
    fill = has_rows if rows.metric == "dot" else np.zeros_like(has_rows)
    return np.where(dead, fill, eight)


def keeps(rows, qs, tau, slack=0.0):
    """For thresholds tau [B] on the canonical score: (six, both) bool [nblk * 32, B] — the pairs the 6-bit test keeps, and the
    subset the int8 test (keep_int8) keeps as well."""
    tau = np.asarray(tau, dtype=np.float64)
    sgn, a = (1.0 if slack >= 0 else -1.0), abs(slack)
    s = rows.block_of_rows(rows.s_blk.astype(np.float64))[:, None]   # NaN: no comparison succeeds
    sq = qs.s_q.astype(np.float64)[None, :]
    with np.errstate(invalid="ignore"):
        ssq = s * sq
        rhs = ssq * tau[None, :]
        t2 = ssq * (qs.norm2[None, :] * rows.block_of_rows(rows.r_blk)[:, None] + qs.err2[None, :] * rows.block_of_rows(rows.n_blk)[:, None])
        M = (252.0 * qs.qabs + 126.5 * np.abs(qs.qsum))[None, :]
        L = 4.0 * (rows.u @ qs.qh.T) - 126.5 * qs.qsum[None, :] + t2
        allow = a * (ssq * qs.unit[None, :] + np.abs(rhs) + t2) + min(a, WN_SLACK) * M
        six = L - rhs >= -sgn * allow
    dead = (qs.s_q == 0)[None, :]
    has_rows = ~np.isnan(s)
    fill = has_rows if rows.metric == "dot" else np.zeros_like(has_rows)
    six = np.where(dead, fill, six)
    return six, six & keep_int8(rows, qs, tau, slack)


def range_tau(bounds, queries, rows):
    """RangeRec::tau of each bound on the reported f32 score (searcher_calls.cpp, range_rec): its canonical value, rounded towards
    "keeps more"; finite bounds only."""
    b = np.asarray(bounds, dtype=np.float32)
    if rows.metric != "dot":
        return np.minimum(np.nextafter(b, np.float32(-np.inf)), np.float32(4.0))
    nq = (np.asarray(queries, dtype=np.float64) ** 2).sum(axis=1)
    most = np.nextafter((2.0 * np.sqrt(nq) * rows.max_norm + 1e-30).astype(np.float32), np.float32(np.inf))
    T = rows.D * (1.0 - np.nextafter(b, np.float32(np.inf)).astype(np.float64))
    Tl = T - np.abs(T) * 1e-9
    tau = np.nextafter(Tl.astype(np.float32), np.float32(-np.inf))
    return np.minimum(np.where(b < 0, most, tau), most)


def reported(c, metric, D):
    """the f32 score a hit carries (scan.h, reported_score)"""
    c = np.asarray(c, dtype=np.float64)
    if metric == "dot":
        d = 1.0 - c / np.float64(D)
        return np.where(d > 0.0, d, 0.0).astype(np.float32)
    return c.astype(np.float32)


_range_cases = {}


def range_case(oracle, D, metric, B=64, edges=False, depth=200, shared=0.0):
    """The fixed-threshold case of test_six_paths_gpu.py, once per (D, metric): 3 007 rows, 64 queries with 30 near rows planted for
    each, and per query the reported score of its 60th best row as the bound, so that 20..200 rows are in range.  Returns
    (corpus, queries, bounds, in_range, opos, orep): the oracle's 200 best positions per query and their reported scores.
    The same for B queries (tests/screens_ref.py): as many near rows each as 3 007 rows allow, 30 at the most, a seed of its own,
    the oracle's `depth` best, and with `edges` an all-zero row, a row with an inf and a row with one dominant component
    (EDGE_ROWS; edges = "blocks": a row with a dominant component in every block).  shared > 0: every row carries N(0, shared^2)
    times one common direction and every query +-shared times it, so that a query's scores spread far wider than 1 / sqrt(D) and
    few rows lie within a rounding's reach of any bound.  The defaults draw what they always drew."""
    key = (D, metric) if (B, edges, depth, shared) == (64, False, 200, 0.0) else (D, metric, B, edges, depth, shared)
    if key in _range_cases:
        return _range_cases[key]
    rng = np.random.default_rng(6000 + D + (1 if metric == "dot" else 0) + (0 if len(key) == 2 else 100_000 + 7 * B))
    n, near = 3007, min(30, 3007 // B)
    queries = rng.standard_normal((B, D)).astype(np.float32)
    corpus = rng.standard_normal((n, D))
    if shared > 0:
        u = rng.standard_normal(D)
        queries = (queries + shared * rng.choice([-1.0, 1.0], (B, 1)) * u[None, :]).astype(np.float32)
        corpus = corpus + shared * rng.standard_normal((n, 1)) * u[None, :]
    spots = rng.permutation(n)[: B * near].reshape(B, near)
    for q in range(B):  # cosines of 0.1 .. 0.45 with their query
        w = rng.uniform(0.1, 0.5, (near, 1))
        corpus[spots[q]] = w * queries[q][None, :] + corpus[spots[q]]
    corpus = (corpus * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    if edges:
        zero, inf, dominant = EDGE_ROWS
        corpus[zero] = 0.0
        corpus[inf, 3] = np.inf
        corpus[dominant] *= np.float32(0.01)
        corpus[dominant, 0] = 20.0  # one component far above the rest of its block
        if edges == "blocks":  # ... and one such row in every block: the block scales are those of one-hot rows
            for b in range(0, n, 32):
                r = min(b + 7, n - 1)
                if r not in EDGE_ROWS:
                    corpus[r] *= np.float32(0.01)
                    corpus[r, (b // 32) % D] = 20.0
    opos, sc, cnt = oracle.topk(queries, corpus, depth, metric=1 if metric == "dot" else 0)
    assert (cnt == depth).all()
    orep = reported(sc, metric, D)
    bounds = orep[:, 59].copy()
    in_range = (orep <= bounds[:, None]).sum(1) if metric == "dot" else (orep >= bounds[:, None]).sum(1)
    assert (in_range >= 20).all() and (in_range < 200).all()
    _range_cases[key] = (corpus, queries, bounds, in_range, opos, orep)
    return _range_cases[key]


EDGE_ROWS = (77, 1490, 2050)  # range_case(edges=True): the all-zero row, the row with an inf, the row with a dominant component
