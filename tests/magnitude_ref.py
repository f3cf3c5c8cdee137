"""Magnitudes (DESIGN.md "Magnitudes"): case builders over the whole range of row and query magnitudes the contract of
include/perceive_hip.h admits, and `envelope`, the f32 quantities the kernels form from a case, evaluated in numpy f32 operation
for operation.  CPU only: float64 and numpy f32.

The invariance every "inside" case rests on: f32 x f32 is exact in f64, so a row or query times a power of two leaves the
canonical cosine (oracle/scan.c, orc_canonical_score) unchanged bit for bit and multiplies the canonical dot by exactly that
power, as long as every scaled value stays a normal f32.  On the device the row scale (float)(1 / sqrt(nx)) then scales by the
exact inverse wherever it is a normal f32, y = x * scale is the same bits, and so is every screening copy."""
import numpy as np

F32_MAX = np.float32(np.finfo(np.float32).max)
F32_TINY = np.float32(np.finfo(np.float32).tiny)  # 2^-126, the smallest normal
SHAPES = {96: 3007, 384: 3007, 1024: 1000}  # D -> rows: 93 full blocks and a partial one; 96 is padded to 128 features
NQ = 64
WIDE_ROW_EXP = (-62, 120)
WIDE_QUERY_EXP = (-60, 99)
DOT_UNIFORM = [(-30, -40), (-60, -60), (40, 40), (20, -20)]
_base = {}


def base(D):
    """(rows [n, D], queries [64, D]): Gaussian f32, fixed seeds"""
    if D not in _base:
        rng = np.random.default_rng(77_000 + D)
        rows = rng.standard_normal((SHAPES[D], D)).astype(np.float32)
        queries = rng.standard_normal((NQ, D)).astype(np.float32)
        rows.setflags(write=False)
        queries.setflags(write=False)
        _base[D] = (rows, queries)
    return _base[D]


def is_normal(a):
    a = np.abs(np.asarray(a, dtype=np.float32))
    return np.isfinite(a) & (a >= F32_TINY)


def scale_pow2(a, e):
    """a[i] * 2^e[i] per row, in f32; every nonzero result is a normal f32 and equals the float64 product exactly"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    e = np.broadcast_to(np.asarray(e, dtype=np.int32).reshape(-1, 1), a.shape)
    out = np.ldexp(a, e).astype(np.float32)
    nz = a != 0
    assert is_normal(out[nz]).all() and (out[~nz] == 0).all()
    assert (out.astype(np.float64) == np.ldexp(a.astype(np.float64), e)).all()
    return out


def scaled_rows(D, e):
    return scale_pow2(base(D)[0], e)


def scaled_queries(D, e):
    return scale_pow2(base(D)[1], e)


def wide_exponents(n, lo, hi, seed):
    """uniform in lo..hi; the first two rows of every 32-row block hold the two ends, so one block spans the whole range"""
    e = np.random.default_rng(seed).integers(lo, hi + 1, n).astype(np.int32)
    e[0::32] = lo
    e[1::32] = hi
    return e


def cosine_wide(D):
    """-> (rows, queries, row exponents, query exponents): base rows and queries times per-row / per-query powers of two"""
    n = SHAPES[D]
    er = wide_exponents(n, *WIDE_ROW_EXP, seed=1 + D)
    eq = wide_exponents(NQ, *WIDE_QUERY_EXP, seed=2 + D)
    return scaled_rows(D, er), scaled_queries(D, eq), er, eq


def wide_queries(D, B):
    """-> (plain [B, D], scaled [B, D]) for B up to 128: the base queries, then the same vectors with their features rotated by one
    place; scaled = plain times per-query powers of two in WIDE_QUERY_EXP"""
    q = base(D)[1]
    plain = np.concatenate([q, np.roll(q, 1, axis=1)])[:B]
    eq = np.concatenate([cosine_wide(D)[3], wide_exponents(NQ, *WIDE_QUERY_EXP, seed=4 + D)[::-1]])[:B]
    return np.ascontiguousarray(plain), scale_pow2(plain, eq)


def other_exponents(D):
    """a second set of row exponents, different from cosine_wide's in every row (update_items moves rows to them)"""
    n = SHAPES[D]
    er = cosine_wide(D)[2]
    e2 = wide_exponents(n, *WIDE_ROW_EXP, seed=3 + D)[::-1].copy()
    same = e2 == er
    e2[same] = np.where(er[same] > 0, er[same] - 17, er[same] + 17)
    return e2


# ---- cosine "edge" rows ------------------------------------------------------------------------------------------------------------
class Edge:
    """Edge rows planted at known positions of the base rows, and the queries that go with them."""

    # name -> (position, searchable)
    ROWS = {
        "norm_at_boundary": (40, True),      # nx = 2^-126 exactly: one feature 2^-63
        "norm_below_boundary": (41, False),  # that feature one ulp lower
        "norm_above_subnormal_rest": (75, True),  # that feature one ulp higher, every other feature a subnormal f32
        "all_subnormal": (76, False),
        "norm_2p126_5": (200, True),         # |x| = 2^126.5, 2^128, 2^130: the row scale is a subnormal f32
        "norm_2p128": (977, True),
        "norm_2p130": (978, True),
        "norm_largest": (999, True),         # features 0.9 * FLT_MAX with random signs: the largest norm the width allows
    }
    LARGE = ("norm_2p126_5", "norm_2p128", "norm_2p130", "norm_largest")

    def __init__(self, D):
        self.D = D
        rng = np.random.default_rng(88_000 + D)
        rows = base(D)[0].copy()
        pos = {k: v[0] for k, v in self.ROWS.items()}
        one = np.float32(2.0 ** -63)
        j = 5
        rows[pos["norm_at_boundary"]] = 0
        rows[pos["norm_at_boundary"], j] = one
        rows[pos["norm_below_boundary"]] = 0
        rows[pos["norm_below_boundary"], j] = np.nextafter(one, np.float32(0))
        sub = (rng.integers(1, 1 << 23, D).astype(np.uint32)).view(np.float32) * rng.choice(np.float32([-1, 1]), D)
        assert (np.abs(sub) < F32_TINY).all() and (sub != 0).all()
        rows[pos["norm_above_subnormal_rest"]] = sub
        rows[pos["norm_above_subnormal_rest"], j] = np.nextafter(one, np.float32(1))
        rows[pos["all_subnormal"]] = sub[::-1]
        for name, lg in (("norm_2p126_5", 126.5), ("norm_2p128", 128.0), ("norm_2p130", 130.0)):
            v = rows[pos[name]].astype(np.float64)
            big = v * (2.0 ** lg / np.sqrt((v * v).sum()))
            assert np.abs(big).max() < float(F32_MAX), (name, D)
            rows[pos[name]] = big.astype(np.float32)
        rows[pos["norm_largest"]] = np.float32(0.9) * F32_MAX * rng.choice(np.float32([-1, 1]), D)
        assert np.isfinite(rows).all()
        self.rows, self.pos = rows, pos
        self.searchable = {k: v[1] for k, v in self.ROWS.items()}
        # queries: both sides of nq = 2^-126, one with |q| > 2^126, a plain one, then per large row a near copy
        q = [np.zeros(D, np.float32), np.zeros(D, np.float32)]
        q[0][j + 1] = one                                   # live: its cosine with a row is that row's feature j + 1 over |x|
        q[1][j + 1] = np.nextafter(one, np.float32(0))      # dead: count 0
        v = base(D)[1][0].astype(np.float64)
        q.append((v * (2.0 ** 127 / np.sqrt((v * v).sum()))).astype(np.float32))
        q.append(base(D)[1][1].copy())
        self.live = [True, False, True, True]
        self.near_copy = {}
        for name in self.LARGE:
            r = rows[pos[name]].astype(np.float64)
            noise = rng.standard_normal(D) * (0.02 * np.sqrt((r * r).sum() / D))
            c = (0.5 * (r + noise)).astype(np.float32)  # (half the row: the noise cannot push a feature past FLT_MAX)
            assert np.isfinite(c).all()
            self.near_copy[name] = len(q)
            q.append(c)
            self.live.append(True)
        self.queries = np.ascontiguousarray(np.stack(q), dtype=np.float32)

    def near_rank_queries(self, oracle, k):
        """per large row a query (a plain query plus t times the row's direction) for which the oracle ranks the row at k - 2 .. k + 1
        (0-based), i.e. at the edge of a top-k list; t by bisection on float64 cosines, the rank then read from the oracle"""
        D = self.D
        r64 = self.rows.astype(np.float64)
        n2 = (r64 * r64).sum(1)
        ok = (n2 >= 2.0 ** -126) & np.isfinite(n2)
        unit = np.where(ok[:, None], r64 / np.sqrt(np.where(ok, n2, 1.0))[:, None], 0.0)
        out = {}
        for i, name in enumerate(self.LARGE):
            p = self.pos[name]
            u = base(D)[1][10 + i].astype(np.float64)
            u /= np.sqrt((u * u).sum())

            def rank(t):
                qv = u + t * unit[p]
                c = unit @ qv
                return int(((c > c[p]) & ok).sum())

            lo, hi = 0.0, 2.0
            assert rank(lo) > k and rank(hi) == 0
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                if rank(mid) >= k - 1:
                    lo = mid
                else:
                    hi = mid
            qv = (u + lo * unit[p]).astype(np.float32)
            opos, _, _ = oracle.topk(qv[None, :], self.rows, k + 4)
            at = np.flatnonzero(opos[0] == p)
            assert at.size == 1 and k - 2 <= at[0] <= k + 1, (name, at)
            out[name] = qv
        return out


_edges = {}


def cosine_edge(D):
    if D not in _edges:
        _edges[D] = Edge(D)
    return _edges[D]


# ---- dot cases ---------------------------------------------------------------------------------------------------------------------
def dot_uniform(D, a, b):
    n = SHAPES[D]
    return scaled_rows(D, np.full(n, a)), scaled_queries(D, np.full(NQ, b))


MIXED_BIG_ROW, MIXED_SMALL_BLOCK = 834, 17


def dot_mixed(D):
    """plain rows, one row times 2^40 (it sets max_norm for every row), one block times 2^-40"""
    n = SHAPES[D]
    e = np.zeros(n, np.int32)
    e[MIXED_BIG_ROW] = 40
    e[MIXED_SMALL_BLOCK * 32:(MIXED_SMALL_BLOCK + 1) * 32] = -40
    return scaled_rows(D, e), base(D)[1].copy()


def _with_max_feature(a, lg):
    """every row of a times a power of two and its largest |feature| then set to 2^lg exactly (smaller ones may turn subnormal)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    mx = np.abs(a).max(1)
    e = (lg - 1 - np.floor(np.log2(mx))).astype(np.int32)
    out = np.ldexp(a, e[:, None]).astype(np.float32)
    j = np.abs(a).argmax(1)
    out[np.arange(a.shape[0]), j] = np.sign(a[np.arange(a.shape[0]), j]) * np.float32(2.0 ** lg)
    assert (np.abs(out).max(1) == np.float32(2.0 ** lg)).all()
    return out


SMALL_BLOCK = 50            # rows 1600..1631
SMALL_SEGMENT = (2 * 3007 // 3, None)  # the rows of source 2 as tests/test_magnitude_gpu.py builds a searcher


def dot_outside(D, name):
    """-> (rows, queries, the envelope quantities the case pushes out of f32, sorted).  Each isolates one quantity as far as the
    arithmetic lets it: the margins are multiples of unit and v_q of s_q, so they leave with them."""
    rows, queries = base(D)[0].copy(), base(D)[1].copy()
    if name in ("q_max_2p-121", "q_max_2p-125", "q_max_subnormal"):
        lg = {"q_max_2p-121": -121, "q_max_2p-125": -125, "q_max_subnormal": -130}[name]
        queries[:8] = _with_max_feature(queries[:8], lg)
        # 127 / 2^-121 = 1.98 * 2^127 is still finite (the boundary is 127 / FLT_MAX = 3.73e-37, just below 2^-121 = 3.76e-37), but
        # the margins, 2 eps32 |q| max_norm ~ 1e-4 * 2^-116, are subnormal already; below that v_q = 0.5002 l1 s_q follows s_q
        return rows, queries, (["margin32"] if lg == -121 else ["margin", "margin32", "s_q", "t_q", "v_q"])
    if name == "block_max_2p-122":
        rows[SMALL_BLOCK * 32:(SMALL_BLOCK + 1) * 32] = _with_max_feature(rows[SMALL_BLOCK * 32:(SMALL_BLOCK + 1) * 32], -122)
        return rows, queries, ["s_blk", "s_mid"]
    if name == "segment_max_2p-122":
        rows[SMALL_SEGMENT[0]:] = _with_max_feature(rows[SMALL_SEGMENT[0]:], -122)
        return rows, queries, ["s_blk", "s_mid"]
    if name == "margin_2p129":
        # |q| max|x| just above FLT_MAX for every query, sum |q_i x_i| <= 0.8 |q||x| (Gaussian: ~0.64) below it for every pair
        r64, q64 = rows.astype(np.float64), queries.astype(np.float64)
        nr, nq = np.sqrt((r64 * r64).sum(1)), np.sqrt((q64 * q64).sum(1))
        f = np.sqrt(1.02 * float(F32_MAX) / (nq.min() * nr.max()))
        rows, queries = (r64 * f).astype(np.float32), (q64 * f).astype(np.float32)
        return rows, queries, ["margin", "margin32", "t_q", "unit"]
    if name == "threshold_2p129":
        # rows times 2^118, queries times 2^-20: unit ~ 2^107 is accepted, T_q ~ 127 * 5.6 * 2^122 is past FLT_MAX
        n = SHAPES[D]
        return scaled_rows(D, np.full(n, 118)), scaled_queries(D, np.full(NQ, -20)), ["t_q"]
    if name == "products_overflow":
        n = SHAPES[D]
        return scaled_rows(D, np.full(n, 70)), scaled_queries(D, np.full(NQ, 70)), ["accumulator", "margin", "margin32", "t_q", "unit"]
    raise KeyError(name)


DOT_OUTSIDE = ["q_max_2p-121", "q_max_2p-125", "q_max_subnormal", "block_max_2p-122", "segment_max_2p-122", "margin_2p129",
               "products_overflow", "threshold_2p129"]


# ---- the envelope ------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _state(v, must_be_nonzero=True):
    """finite / normal / nonzero of every element of v -> one dict; `ok`: all finite, and normal and nonzero where required"""
    v = _f32(v)
    finite = bool(np.isfinite(v).all())
    nonzero = bool((v != 0).all())
    normal = bool((is_normal(v) | (v == 0)).all())
    return {"finite": finite, "normal": normal, "nonzero": nonzero, "ok": finite and normal and (nonzero or not must_be_nonzero)}


def row_scale(rows, metric):
    """corpus_kernels.hip row_scale (:55-59): nx in f64 in feature order; cosine (float)(1 / sqrt(nx)) for finite nx >= 2^-126, dot 1
    for finite nx; 0 otherwise.  -> (scale f32 [n], nx f64 [n])"""
    r = np.ascontiguousarray(rows, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        nx = np.cumsum(r * r, axis=1)[:, -1]
    finite = nx < np.inf
    if metric == "dot":
        return np.where(finite, np.float32(1), np.float32(0)).astype(np.float32), nx
    ok = finite & (nx >= 2.0 ** -126)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = (1.0 / np.sqrt(np.where(ok, nx, 1.0))).astype(np.float32)
    return np.where(ok, sc, np.float32(0)).astype(np.float32), nx


def envelope(rows, queries, metric, D):
    """The f32 quantities the kernels form from (rows, queries), each with _state's verdict, and `inside`: all of them are ok.

      row_scale    corpus_kernels.hip:55-59 (row_scale), searchable rows only
      unit         scan_kernels.hip:329 and :460 (both seed kernels): (float)sqrt(sum) * max_norm * 1.0001f; cosine 1.
                   max_norm: corpus_kernels.hip:61-66 (raise_max_norm), (float)sqrt(nx) * 1.000001f over the searchable rows
      margin       scan_kernels.hip:330 / :461, (eps16 + eps32) * unit;  margin32: :331 / :462, 2 * eps32 * unit;
                   eps32 = (Dp + 16) * 1.2e-7f, eps16 = 0.0039101f + 2 eps32 (searcher_pass.cpp:172-173)
      s_q          scan_kernels.hip:1062 (quantize_queries_kernel), 127.0f / max|q'_i|, live queries with a nonzero feature
      v_q          scan_kernels.hip:1087, 0.5002f * l1 * s_q + 0.2501f * Dp8 + 4
      t_q          int8_threshold (scan_kernels.hip), (tau - e32) * s_q at its largest, tau = unit: 127 (|q| / max|q_i|) max_norm,
                   whatever the query's own scale; the kernels cap it at FLT_MAX, and c1 = 0.5002f * sqrt(Dp8) * max_norm beside it
      s_blk        corpus_kernels.hip:108 (pack8_block), 127.0f / bm, bm the largest |x_i * scale| of a block's searchable rows
      s_mid        corpus_kernels.hip:137 (mid_block_scale), s_blk * (32766.0f / 127.0f), and :164 (mid_pack_row), 32766.0f / mx
      accumulator  the largest |partial sum| an f32 accumulator of q'.x can reach, bounded by sum |q'_i x_i| (f64); the wave kernel
                   and the seeds accumulate over the unscaled row (scan_kernels.hip:364 prep_seed_kernel, :608 scan_wave_kernel, screen_score afterwards)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    Dp = (D + 63) // 64 * 64
    Dp8 = (Dp + 127) // 128 * 128
    out = {}
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        scale, nx = row_scale(rows, metric)
        live_rows = scale != 0
        out["row_scale"] = dict(_state(scale[live_rows]), value=scale)
        max_norm = (np.sqrt(nx[live_rows]).astype(np.float32) * np.float32(1.000001)).max() if live_rows.any() else np.float32(0)
        q64 = queries.astype(np.float64)
        nq = np.cumsum(q64 * q64, axis=1)[:, -1]
        if metric == "dot":
            live_q = nq < np.inf
            inv = np.ones(len(queries), np.float32)
            unit = np.sqrt(nq).astype(np.float32) * max_norm * np.float32(1.0001)
        else:
            live_q = (nq >= 2.0 ** -126) & (nq < np.inf)
            inv = np.where(live_q, (1.0 / np.sqrt(np.where(live_q, nq, 1.0))).astype(np.float32), np.float32(0)).astype(np.float32)
            unit = np.ones(len(queries), np.float32)
        eps32 = np.float32(Dp + 16) * np.float32(1.2e-7)
        eps16 = np.float32(0.0039101) + np.float32(2) * eps32
        some_q = live_q & (nq > 0)  # an all-zero dot query has unit 0 by design
        out["inv_q"] = dict(_state(inv[live_q]), value=inv)
        out["unit"] = dict(_state(unit[some_q]), value=unit)
        out["margin"] = dict(_state(((eps16 + eps32) * unit)[some_q]), value=(eps16 + eps32) * unit)
        out["margin32"] = dict(_state((np.float32(2) * eps32 * unit)[some_q]), value=np.float32(2) * eps32 * unit)
        qp = np.where(live_q[:, None], queries * inv[:, None], np.float32(0)).astype(np.float32)
        mx = np.abs(qp).max(1)
        l1 = np.abs(qp).sum(1, dtype=np.float32)
        s_q = np.float32(127) / mx
        v_q = np.float32(0.5002) * l1 * s_q + np.float32(0.2501) * np.float32(Dp8) + np.float32(4)
        has = some_q & (mx > 0)
        out["s_q"] = dict(_state(s_q[has]), value=s_q)
        # T_q <= unit * s_q: the largest threshold of the int8 / 6-bit tests in units of the quantised query (tau <= |q| max|x|)
        t_q = (unit * s_q).astype(np.float32)
        out["t_q"] = dict(_state(t_q[has]), value=t_q)
        out["v_q"] = dict(_state(v_q[has]), value=v_q)
        y = np.where(live_rows[:, None], rows * scale[:, None], np.float32(0)).astype(np.float32)
        n = rows.shape[0]
        pad = (-n) % 32
        ymax = np.concatenate([np.abs(y).max(1), np.zeros(pad, np.float32)]).reshape(-1, 32)
        bm = ymax.max(1)
        s_blk = (np.float32(127) / bm)[bm > 0]  # (a block of all-zero rows takes s_blk = 1)
        out["s_blk"] = dict(_state(s_blk), value=s_blk)
        row_mx = np.abs(y).max(1)
        s_mid = np.concatenate([s_blk * (np.float32(32766) / np.float32(127)), (np.float32(32766) / row_mx)[row_mx > 0]])
        out["s_mid"] = dict(_state(s_mid), value=s_mid)
        acc = (np.abs(qp).astype(np.float64) @ np.abs(np.where(live_rows[:, None], rows, 0)).astype(np.float64).T).max() if n else 0.0
        out["accumulator"] = {"finite": bool(acc <= float(F32_MAX)), "normal": True, "nonzero": True, "ok": bool(acc <= float(F32_MAX)),
                              "value": acc}
    out["inside"] = all(v["ok"] for v in out.values())
    out["outside"] = sorted(k for k, v in out.items() if isinstance(v, dict) and not v["ok"])
    return out

