"""A float64 numpy model of the screens the 6-bit model of tests/six_ref.py leaves out, written from the kernels of
csrc/scan_kernels.hip and the copies of csrc/corpus_kernels.hip, and a mirror of the launchers that tells which kernel form a
pass reaches.  TEST INFRASTRUCTURE ONLY: tests/test_screens_cpu.py checks the models' certificates, the width of their brackets
and that SHAPES reach every form; tests/test_screens_gpu.py holds the device's survivor counts of range passes against them.

Every keep_* function returns bool [nblk * 32, B]: the (row, query) pairs the screen keeps for thresholds tau [B] on the canonical
score.  `slack` loosens the test when positive and tightens it when negative; each *_slack(D) is the value that covers what the
kernel's arithmetic may add, derived in its docstring from the kernel text.  Nothing here is fitted to a device count.

  keep_int8   scan_mfma8_kernel / scan_mfma8_hold_kernel: six_ref.keep_int8, the one copy of that test
  keep_bf16   scan_mfma_kernel, from the bf16 copy (bf16_piece) or from the f32 rows converted in the loop
  keep_mid    the mid copy's test, written twice on the device: fine_survivors and drain_survivors
  keep_fine   the f32 score's test: fine_survivors, drain_survivors, scan_wave_kernel
  scan_form   launch_scan_mfma8, launch_scan_mfma, launch_scan_wave, mfma8_pass_queries, mfma_pass_queries, mfma8_six_pass
"""
from collections import namedtuple

import numpy as np

import six_ref
from six_ref import Queries, Rows, eps32, keep_int8, range_tau, reported  # noqa: F401  (the model's other half)

F32 = np.float32


# ---- the query constants prep_seed* writes ------------------------------------------------------------------------------------------
def margins(rows, qs):
    """(margin, margin32) [B] as prep_seed_kernel / prep_seed_mfma_kernel write them, in f32 arithmetic: (eps16 + eps32) unit and
    2 eps32 unit with eps32 = (Dp + 16) 1.2e-7, eps16 = 0.0039101 + 2 eps32 (searcher_pass.cpp, fill_params) and unit = 1 (cosine) or
    (float)|q| max_norm 1.0001 (dot)."""
    e32 = F32(rows.Dp + 16) * F32(1.2e-7)
    e16 = F32(0.0039101) + F32(2.0) * e32
    if rows.metric == "dot":
        nq = (qs.unit / rows.max_norm if rows.max_norm > 0 else np.zeros(qs.B)).astype(F32)
        unit = nq * F32(rows.max_norm) * F32(1.0001)
    else:
        unit = np.ones(qs.B, F32)
    return ((e16 + e32) * unit).astype(np.float64), (F32(2.0) * e32 * unit).astype(np.float64)


def bf16(x):
    """f32 -> bf16 by round-to-nearest-even (what (__bf16)x and __builtin_convertvector do), returned as f32"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    r = u >> np.uint32(16)  # u + 0x7FFF + ((u >> 16) & 1), cut to the high half: one array, worked in place
    r &= np.uint32(1)
    r += np.uint32(0x7FFF)
    r += u
    r &= np.uint32(0xFFFF0000)
    return r.view(F32)


def _memo(rows, qs, name, make):
    """products that do not depend on the thresholds, once per (rows, queries)"""
    store = rows.__dict__.setdefault("_screens_memo", {})
    key = (name, id(qs))
    if key not in store:
        store[key] = (qs, make())  # (the queries are held: their id stays theirs)
    return store[key][1]


def _split(slack):
    return (1.0 if slack >= 0 else -1.0), abs(slack)


# ---- the int8 test ------------------------------------------------------------------------------------------------------------------
def int8_slack(D):
    """What scan_mfma8_kernel's epilogue (and u_of of the DRAIN and hold forms, the same lines) adds to six_ref.keep_int8, each
    relative to a quantity that test's slack multiplies (s_blk s_q unit, |Rhs|, s_blk c1, V_q):
      - e32 = margin32 / 2 = eps32 unit (dot: with the unit's 1.0001) comes off tau first: 1.0001 eps32 of s_blk s_q unit;
      - T = (tau - e32) s_q is lowered by 2e-6 |T|: 2e-6 of |Rhs| and of s_blk s_q unit;
      - f32 roundings: two in T, one in T - 2e-6 |T|, one in - c1, one in fmaf(s_blk, U, -V), three in V_q's own expression
        (quantize_queries_kernel) and three in c1 = 0.5002 sqrtf(Dp8) nrm: at most four of 2^-24 on any one term, 2^-22.
    acc8 is an exact integer below 2^24, so (float)acc8 adds nothing."""
    return 1.0001 * eps32(D) + 2e-6 + 2.0 ** -22


# ---- the bf16 screen ----------------------------------------------------------------------------------------------------------------
def bf16_slack(D):
    """scan_mfma_kernel keeps a pair iff !(acc < thr), thr = key_f32(tau) - margin in f32, acc = the MFMA's f32 sum of the Dp
    products bf16(y_i) bf16(q'_i).  Each product of two 8-bit significands is exact in f32; only the order of the Dp additions is
    the hardware's.  Any order of n f32 additions errs by at most (n - 1) 2^-24 sum |y_i q'_i| <= (n - 1) 2^-24 |y^|_2 |q^|_2,
    and the bf16 rounding grows each norm by at most 1 + 2^-8: below Dp 6.1e-8 unit, half of eps32(D) unit = (Dp + 16) 1.2e-7 unit,
    the bound the project claims for such a chain.  The threshold: one rounding of the subtraction, 2^-24 |thr|, and two in the
    margin's own product, 2^-23 margin < 2^-24 unit.  So: eps32(D) of unit, 2^-23 of unit + |thr|."""
    return eps32(D) + 2.0 ** -23


def keep_bf16(rows, qs, tau, slack=0.0, f32_rows=False):
    """s16 = sum bf16(y_i) bf16(q'_i) with y = x scale the f32 product (bf16_piece; `v * sc_cur` in the loop) and q' as prep_seed*
    writes qbf16; kept iff !(s16 < tau - margin).  Rows without a scale and the padding of the last block are zeros in the copy:
    they pass whenever tau - margin <= 0.  f32_rows (SRC16 = false, no copy): the loop multiplies the row as it is stored by its
    scale, so a row with an inf or a NaN (scale 0) gives NaN accumulators for every query of the pass, and !(NaN < thr) holds:
    the kernel counts it as a coarse survivor and sheds it at its scale in fine_survivors.  Slack: allow = |slack| (unit + |thr|)."""
    tau = np.asarray(tau, dtype=np.float64)
    sgn, a = _split(slack)
    s16 = _memo(rows, qs, "s16", lambda: bf16(rows.y32).astype(np.float64) @ bf16(qs.qp.astype(F32)).astype(np.float64).T)
    thr = (tau - margins(rows, qs)[0])[None, :]
    keep = ~(s16 < thr - sgn * a * (qs.unit[None, :] + np.abs(thr)))
    if f32_rows:
        keep = keep | rows.nonfinite[:, None]
    return keep


# ---- the mid test -------------------------------------------------------------------------------------------------------------------
def mid_slack(D, reader="drain_survivors"):
    """Both copies of the test compute part = sum q'_i Y_i in f32 and then part / s2 >= taum - (quant + 1.5 m32).  The band quant
    is some 1e-4 of a score, the size of eps32 itself, so a slack of eps32 would hide any error in it; the sum's own order gives
    a far closer bound.  A sum taken along a tree of additions errs by at most depth 2^-24 / (1 - depth 2^-24) of sum |q'_i Y_i|,
    depth = the most roundings any one term goes through, and sum |q'_i Y_i| / s2 <= |q'|_2 |Y|_2 / s2 <= unit (1 + 2^-15):
      - fine_survivors: lane l of 64 takes the 16-byte pieces l, l + 64, ... of the Dp / 8, eight FMAs a piece in one chain,
        then a butterfly of six additions: depth = 8 ceil(Dp / 512) + 6;
      - drain_survivors: lane `sub` of 8 takes the pieces sub, sub + 8, ... (three a round, one chain), then three additions:
        depth = 8 ceil(Dp / 64) + 3.
    The rest is single roundings: the division, quant = l1 0.5003f / s2 (two), 1.5 m32, the sum and the subtraction — five of
    2^-24, each on |tau|, part / s2 (<= unit) or the band: 2^-22 of their sum covers them.  l1 is an f32 sum in lane order on the
    device and in feature order in the model: (Dp + 6) 2^-24 of quant (1e-4 of unit), below 2^-24 of unit.  So:
    (depth + 1) 2^-24 (1 + 2^-14) + 2^-22, of unit + |tau| + quant + 1.5 m32."""
    Dp = six_ref.padded(D)[0]
    depth = {"fine_survivors": 8 * -(-Dp // 512) + 6, "drain_survivors": 8 * -(-Dp // 64) + 3}[reader]
    return (depth + 1) * 2.0 ** -24 * (1 + 2.0 ** -14) + 2.0 ** -22


def mid_codes(rows):
    """(Y [nblk * 32, Dp] f64, s2 [nblk * 32] f64): the codes rint(y s2) clamped to +-32767 (mid_pair; the product is an f32 one)
    and s2 = s_blk (32766 / 127) in f32 (mid_block_scale), NaN for a block without a searchable row"""
    if "_screens_mid" not in rows.__dict__:
        s2 = (rows.s_blk.astype(F32) * (F32(32766.0) / F32(127.0))).astype(F32)
        s2r = rows.block_of_rows(s2)
        safe = np.where(np.isnan(s2r), F32(0.0), s2r).astype(F32)
        Y = np.clip(np.rint(rows.y32 * safe[:, None]), -32767, 32767).astype(np.float64)
        Y[rows.scale == 0] = 0.0
        rows._screens_mid = (Y, s2r.astype(np.float64))
    return rows._screens_mid


def keep_mid(rows, qs, tau, slack=0.0):
    """The mid test of a coarse survivor with sc != 0: kept iff part / s2 >= tau - (|q'|_1 0.5003f / s2 + 1.5 margin32), part =
    sum q'_i Y_i.  A row without a scale is dropped before the test (`if (sc == 0.0f) continue`, `go = on && sc != 0.0f`), a NaN
    s2 fails the comparison.  Slack: allow = |slack| (unit + |tau| + quant + 1.5 margin32)."""
    tau = np.asarray(tau, dtype=np.float64)
    sgn, a = _split(slack)
    Y, s2 = mid_codes(rows)
    part = _memo(rows, qs, "mid", lambda: Y @ qs.qp.T)
    with np.errstate(invalid="ignore", divide="ignore"):
        band = (qs.l1[None, :] * np.float64(F32(0.5003))) / s2[:, None] + 1.5 * margins(rows, qs)[1][None, :]
        allow = a * (qs.unit[None, :] + np.abs(tau)[None, :] + band)
        keep = part / s2[:, None] >= tau[None, :] - band - sgn * allow
    return keep & (rows.scale != 0)[:, None]


# ---- the fine test ------------------------------------------------------------------------------------------------------------------
def fine_slack(D):
    """s32 = dot * sc with dot an f32 FMA chain over the Dp features in the kernel's own order (wave_dot_f32: 64 lanes and a
    butterfly; drain_survivors: 8 lanes; scan_wave_kernel: two half rows): |dot sc - s32| <= eps32(D) unit, the bound the project
    claims for an f32 FMA chain in any order (searcher_pass.cpp, fill_params) — Dp 2^-24 is half of it, the product with sc and the
    subtraction tau - margin32 take 2^-24 of |s32| <= unit and of |tau|.  So: eps32(D) + 2^-23 of unit + |tau|."""
    return eps32(D) + 2.0 ** -23


def keep_fine(rows, qs, tau, slack=0.0):
    """kept iff s32 >= tau - margin32 and scale != 0; s32 = the f64 dot of q' with the f32 row, times the row's scale.  (The
    kernels write !(s32 < ...); s32 is finite for every row that has a scale.)  Slack: allow = |slack| (unit + |tau|)."""
    tau = np.asarray(tau, dtype=np.float64)
    sgn, a = _split(slack)
    s32 = _memo(rows, qs, "s32", lambda: (rows.x @ qs.qp.T) * rows.scale.astype(np.float64)[:, None])
    thr = (tau - margins(rows, qs)[1])[None, :]
    return (s32 >= thr - sgn * a * (qs.unit[None, :] + np.abs(tau)[None, :])) & (rows.scale != 0)[:, None]


# ---- which kernel a pass reaches ------------------------------------------------------------------------------------------------------
FLAG_PLAIN, FLAG_TILE128, FLAG_FOUR_WAVE, TUNE_NO_SIX = 1 << 0, 1 << 3, 1 << 28, 1 << 29  # scan.h
LDS_ROOM = 156 * 1024

Drain = namedtuple("Drain", "nt ncht nch nbuf ntl")          # scan_mfma8_kernel<NT, NTL, 12, NBUF, true, NCHT>; nch: chunks at run time
Six = namedtuple("Six", "nt ncht")                            # scan_mfma8_kernel<NT, true, 12, 4, true, NCHT, true>
Four = namedtuple("Four", "nt wpb nbuf ntl")                  # scan_mfma8_kernel<NT, NTL, WPB, NBUF>: every wave handles its own survivors
Hold = namedtuple("Hold", "nch nh ntl")                       # scan_mfma8_hold_kernel<NTL, NCH, NH>
Mfma = namedtuple("Mfma", "nt wide src16 nbuf wpb ntl")       # scan_mfma_kernel<NT, NTL, WPB, NBUF, SRC16>
Wave = namedtuple("Wave", "nb ntl")                           # scan_wave_kernel<NB, NTL>


def chunk_bufs(flags):
    return (flags >> 24) & 0xF  # scan.h: flags_chunk_bufs


def mfma_pass_queries(Dp):
    for nt in (4, 2, 1):  # mfma_pass_queries: the bf16 tile of 32 nt rows must fit
        if nt * 32 * Dp * 2 <= LDS_ROOM:
            return nt * 32
    return 0


def mfma8_lds(nt, Dp):
    return nt * 32 * ((((Dp + 127) & ~127) >> 4) + 1) * 16  # mfma8_lds


def mfma8_pass_queries(Dp):
    if ((Dp + 127) & ~127) <= 384:  # mfma8_pass_queries: the block-holding form, four halves
        return 256
    for nt in (4, 2, 1):
        if mfma8_lds(nt, Dp) <= LDS_ROOM:
            return nt * 32
    return 0


def six_pass(B, Dp, flags, nseg):
    """mfma8_six_pass"""
    nt = 1 if B <= 32 else 2
    return (4 < B <= 64 and ((Dp + 127) & ~127) <= 384 and not flags & FLAG_FOUR_WAVE and not flags & FLAG_PLAIN and chunk_bufs(flags) != 3
            and nseg < (1 << 18) and mfma8_lds(nt, Dp) + 68 * 1024 <= LDS_ROOM)


def scan_form(B, D, flags, screen, nseg=1, six_copy=False):
    """The kernel and template arguments one pass of B queries over rows of D features reaches.  screen: "int8" | "bf16" (the
    copy streamed, MFMA kernel) | "f32" (no copy, set_kernel("mfma")) | "wave" (no copy, AUTO's kernel choice at up to four
    queries); six_copy: every segment has its 6-bit copy and nothing forbids it (fill_segment_table)."""
    Dp = (D + 63) // 64 * 64
    ntl = not flags & FLAG_PLAIN  # launch_scan_*: `ntl = (p.flags & kFlagPlainLoads) == 0`
    if screen == "wave":
        assert B <= 4  # pick_kernel: B <= kMaxWaveQueries without copies
        return Wave(min(B, 4), ntl)  # launch_scan_wave: `switch (p.B)`
    if screen in ("bf16", "f32"):
        assert 0 < B <= mfma_pass_queries(Dp)  # pass_queries
        nt = 1 if B <= 32 else 2 if B <= 64 else 4  # launch_scan_mfma: `const int NT = ...`
        lds = nt * 32 * Dp * 2  # `const size_t lds = ...`
        wide = nt == 4 or lds * 3 > LDS_ROOM  # `const bool wide = ...`
        nbuf = chunk_bufs(flags)
        if screen == "bf16":  # launch_mfma_shape: `if (src16)`
            if nt == 4 or wide:
                return Mfma(nt, wide, True, 4 if nbuf == 4 else 6, 8, ntl)  # `if (nbuf == 4) ... <NT, NTL, 8, 4, true> else <.., 8, 6, true>`
            return Mfma(nt, wide, True, 6 if nbuf == 6 else 4, 4, ntl)  # `if (nbuf == 6) ... <NT, NTL, 4, 6, true> else <.., 4, 4, true>`
        if nt == 4 or wide:
            return Mfma(nt, wide, False, 3, 8, ntl)  # `launch_mfma_variant<NT, NTL, 8, 3, false>`
        return Mfma(nt, wide, False, 2, 4, ntl)  # `launch_mfma_variant<NT, NTL, 4, 2, false>`
    assert screen == "int8" and Dp <= 1024 and 0 < B <= mfma8_pass_queries(Dp)  # fill_segment_table, pass_queries
    nt = 1 if B <= 32 else 2 if B <= 64 else 4 if B <= 128 else 8  # launch_scan_mfma8: `const int NT = ...`
    lds = mfma8_lds(nt, Dp)
    most = 2 if nt == 4 else 3  # `const unsigned most = ...`
    per_cu = max(1, min(most, LDS_ROOM // lds))  # `const unsigned per_cu = ...`
    wide8 = nt == 4 and per_cu == 1  # `const bool wide8 = ...`
    nch = ((Dp + 127) & ~127) >> 7  # `const int nch = ...`
    if B > 64 and nch <= 3 and (B > 128 or not flags & FLAG_TILE128):  # `if (p.B > 64 && nch <= 3 && ...)`: the hold kernel
        return Hold(nch, 4 if B > 128 else 2, ntl)  # `const bool four = p.B > 128`, PCV_HOLD(nch, 4 | 2)
    assert nt != 8  # `if (NT == 8) PCV_FAIL(...)`
    if nt <= 2 and B > 4 and not flags & FLAG_FOUR_WAVE and nseg < (1 << 18) and lds + 68 * 1024 <= LDS_ROOM:  # `if (NT <= 2 && p.B > 4 && ...)`
        if six_copy and not flags & TUNE_NO_SIX and six_pass(B, Dp, flags, nseg):  # `if (p.flags & kFlagSix)`: launch_mfma8_six
            return Six(nt, nch)
        ncht = nch if nch in (1, 2, 3, 4, 6, 8) else 0  # launch_mfma8_drain: `switch (nch)`, `default:` the run-time form
        if nt == 1:
            return Drain(1, ncht, nch, 4, ntl)  # `launch_mfma8_drain<1, ntl, 4>`
        return Drain(2, ncht, nch, 3 if chunk_bufs(flags) == 3 else 4, ntl)  # `if (flags_chunk_bufs(p.flags) == 3) <2, ntl, 3> else <2, ntl, 4>`
    if nt <= 2:
        return Four(nt, 4, 3 if nt == 2 else 4, ntl)  # `launch_mfma8_variant<1 | 2, ntl>`: WPB = 4, NBUF = (NT == 2 ? 3 : 4)
    if wide8:
        return Four(4, 8, 4, ntl)  # `launch_mfma8_variant<4, ntl, 8>`
    return Four(4, 4, 4, ntl)  # `launch_mfma8_variant<4, ntl>`


def mid_reader(form):
    """which copy of the mid test (and of the fine test) a form's coarse survivors meet"""
    return "drain_survivors" if isinstance(form, (Drain, Six)) else "scan_wave_kernel" if isinstance(form, Wave) else "fine_survivors"


# ---- the cases of tests/test_screens_gpu.py -------------------------------------------------------------------------------------------
# One searcher of 3 007 rows per (D, metric, screen, mid, segments); one range pass per Run.  flags: the tuning word;
# every int8 case forbids the 6-bit copy (TUNE_NO_SIX) so that nothing depends on what AUTO builds at this size.
Shape = namedtuple("Shape", "group D B flags screen mid segs")
SEGMENTS = (900, 1, 33, 640, 257, 876, 300)  # seven segments, 3 007 rows: six partial last blocks inside the stream
N8 = TUNE_NO_SIX


def _shapes():
    out = []
    for D in (100, 200, 384, 512, 640, 768, 896, 1024):  # NCHT 1, 2, 3, 4, 0 (5 at run time), 6, 0 (7), 8
        for B in (5, 32, 33, 64):
            out.append(Shape("drain", D, B, N8, "int8", "off", False))
    out += [Shape("drain", D, 64, N8 | (3 << 24), "int8", "off", False) for D in (384, 768)]  # three chunk buffers
    out += [Shape("drain", 200, B, N8 | FLAG_PLAIN, "int8", "off", False) for B in (32, 64)]   # plain loads, once per NT
    for D in (100, 384, 768):
        out += [Shape("four", D, B, N8, "int8", "off", False) for B in (1, 4)]
    out += [Shape("four", 384, B, N8 | FLAG_FOUR_WAVE, "int8", "off", False) for B in (16, 64)]
    out += [Shape("tile128", 512, 65, N8, "int8", "off", False), Shape("tile128", 512, 128, N8, "int8", "off", False),
            Shape("tile128", 768, 128, N8, "int8", "off", False), Shape("tile128", 384, 100, N8 | FLAG_TILE128, "int8", "off", False)]
    for D in (100, 200, 384):
        for B in (65, 100, 128, 129, 200, 256):
            out += [Shape("hold", D, B, N8 | f, "int8", "off", False) for f in (0, FLAG_PLAIN)]
    for D in (100, 384, 768):  # 768-d: two trips of the 16-byte loop
        out += [Shape("mid", D, B, N8, "int8", "on", False) for B in (4, 64, 100, 256) if B <= mfma8_pass_queries((D + 63) // 64 * 64)]
    for D in (100, 384):
        for B in (8, 64, 128):
            out += [Shape("bf16", D, B, nb << 24, "bf16", "off", False) for nb in (4, 6)]
            out.append(Shape("f32rows", D, B, 0, "f32", "off", False))
    out += [Shape("bf16", 512, 64, nb << 24, "bf16", "off", False) for nb in (4, 6)]  # the wide form at NT = 2
    for D in (100, 384):
        out += [Shape("wave", D, B, 0, "wave", "off", False) for B in (1, 4)]
    out += [Shape("segments", 200, 64, N8, "int8", "off", True), Shape("segments", 200, 256, N8, "int8", "off", True)]
    return out


SHAPES = _shapes()
METRICS = ("cosine", "dot")
FEW, RANK, RANK_FEW, DEPTH = 5, 60, 230, 256


def form_of(shape):
    return scan_form(shape.B, shape.D, shape.flags, shape.screen, nseg=len(SEGMENTS) if shape.segs else 1)


def tiles_of(shape):
    """the 32-query tiles a shape's pass has"""
    return (shape.B + 31) // 32


def slacks(D, reader="drain_survivors"):
    return {"int8": int8_slack(D), "bf16": bf16_slack(D), "f32": bf16_slack(D), "mid": mid_slack(D, reader), "fine": fine_slack(D)}


def case_of(oracle, shape, metric):
    """the inputs of a shape: the mid shapes take the rows with a dominant component in every block (Case)"""
    return Case.get(oracle, shape.D, metric, shape.segs, blocks=shape.mid == "on")


class Case:
    """The inputs of every shape at (D, metric) and the model's per-query survivor counts.  six_ref.range_case for 256 queries with
    the edge rows; a pass of B queries takes the first B.  Bounds: the reported score of a query's 60th best row — or, for a query
    whose 32-query tile holds fewer than FEW queries at this B (a tile that is run on its own must still count hundreds of rows,
    see test_screens_cpu.py), of its 230th best; a query that is masked out gets a bound that admits nothing.
    blocks: every block has a row with one dominant component, so that every block scale is that of a one-hot row and the mid
    test's band |q'|_1 0.5003 / s2 is as wide as it gets, some 2.5e-4 of a cosine at 384-d: an error of a tenth in its constant
    then moves mid_survivors by more than the bracket is wide.  (On Gaussian blocks the band is a fifth of that.)"""

    _all = {}

    @classmethod
    def get(cls, oracle, D, metric, segs=False, blocks=False):
        key = (D, metric, segs, blocks)
        if key not in cls._all:
            cls._all[key] = cls(oracle, D, metric, segs, blocks)
        return cls._all[key]

    def __init__(self, oracle, D, metric, segs, blocks):
        self.D, self.metric = D, metric
        self.corpus, self.queries, _, _, self.opos, self.orep = six_ref.range_case(oracle, D, metric, B=256, edges="blocks" if blocks else True,
                                                                                   depth=DEPTH, shared=0.5)
        cuts = np.concatenate([[0], np.cumsum(SEGMENTS)]) if segs else np.array([0, len(self.corpus)])
        assert cuts[-1] == len(self.corpus)
        self.cuts = cuts
        self.parts = [Rows(self.corpus[a:b], metric) for a, b in zip(cuts[:-1], cuts[1:])]
        top = max(r.max_norm for r in self.parts)  # one bound of |x| for the searcher (raise_max_norm)
        for r in self.parts:
            r.max_norm = top
        self.qs = Queries(self.queries, self.parts[0])
        self._counts = {}

    def kinds(self, B, tile=None):
        """per query of the pass: RANK, RANK_FEW, or 0 for a query masked out (tile: the one tile that is not)"""
        q = np.arange(B)
        few = np.minimum(32, B - 32 * (q // 32)) < FEW
        kind = np.where(few, RANK_FEW, RANK)
        return kind if tile is None else np.where(q // 32 == tile, kind, 0)

    def bounds(self, B, tile=None):
        kind = self.kinds(B, tile)
        nothing = F32(-1.0) if self.metric == "dot" else F32(2.0)  # a negative distance; a cosine range_rec caps at 4
        return np.where(kind == 0, nothing, self.orep[np.arange(B), np.maximum(kind, 1) - 1]).astype(F32)

    def in_range(self, B, tile=None):
        b = self.bounds(B, tile)[:, None]
        return ((self.orep[:B] <= b) if self.metric == "dot" else (self.orep[:B] >= b)).sum(1)

    def tau(self, bounds):
        full = np.full(256, bounds[0], F32)
        full[: len(bounds)] = bounds
        return range_tau(full, self.queries, self.parts[0])

    def per_query(self, screen, mid, kind):
        """(lo, hi): dicts of the model's counts per query [256] — "coarse", "mid" (mid: the copy of the mid test that is read,
        fine_survivors | drain_survivors, or None) and "candidates" — with every test tightened / loosened by its slack, for the
        bound kind (RANK, RANK_FEW, 0) given to every query"""
        key = (screen, mid, kind)
        if key in self._counts:
            return self._counts[key]
        tau = self.tau(self.orep[:, kind - 1].astype(F32) if kind else self.bounds(256, tile=-1))
        sl = slacks(self.D, mid or "drain_survivors")
        out = []
        for sgn in (-1.0, 1.0):
            tot = {"coarse": np.zeros(256, np.int64), "candidates": np.zeros(256, np.int64)}
            if mid:
                tot["mid"] = np.zeros(256, np.int64)
            for rows in self.parts:
                fine = keep_fine(rows, self.qs, tau, sgn * sl["fine"])
                if screen == "wave":
                    coarse = np.ones_like(fine)
                elif screen == "int8":
                    coarse = keep_int8(rows, self.qs, tau, sgn * sl["int8"])
                else:
                    coarse = keep_bf16(rows, self.qs, tau, sgn * sl[screen], f32_rows=screen == "f32")
                left = coarse
                if mid:
                    left = coarse & keep_mid(rows, self.qs, tau, sgn * sl["mid"])
                    tot["mid"] += left.sum(0)
                tot["coarse"] += coarse.sum(0)
                tot["candidates"] += (left & fine).sum(0)
            out.append(tot)
        self._counts[key] = tuple(out)
        return self._counts[key]

    def bracket(self, shape, tile=None):
        """{name: (lo, hi)} of the counts one pass of `shape` reports (the wave kernel counts candidates only)"""
        kind = self.kinds(shape.B, tile)
        res = {}
        for k in (RANK, RANK_FEW, 0):
            sel = np.flatnonzero(kind == k)
            if sel.size == 0:
                continue
            lo, hi = self.per_query(shape.screen, mid_reader(form_of(shape)) if shape.mid == "on" else None, k)
            for name in lo:
                a, b = res.get(name, (0, 0))
                res[name] = (a + int(lo[name][sel].sum()), b + int(hi[name][sel].sum()))
        if shape.screen == "wave":
            res.pop("coarse")
        return res
