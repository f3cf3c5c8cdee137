"""A float64 numpy model of the row-pair screens (DESIGN.md §4 "The row-pair screen"), written from the kernels — pair_screen.h and
its policies in selfjoin_, assign_, neighbors_ and linkage_kernels.hip, density_screen_kernel, selfjoin_prep_kernel — and from
the host code that sets their thresholds (row_jobs.cpp).  TEST INFRASTRUCTURE ONLY: tests/test_pairs_cpu.py checks that the brackets
of every case are narrow, that a wrong screen leaves them and that the host mirrors are right; tests/test_pairs_gpu.py holds the
device's candidate counts against them.  Nothing here is fitted to a device count.

The score.  S[a, b] is the screening score in exact arithmetic: the f64 dot product of the two rows rounded to bf16 (round to
nearest even, what __builtin_convertvector does), times the two rinv values as selfjoin_prep_kernel writes them: (float)(1 /
sqrt(n)) of the canonical |x|^2 = n (f64, feature order), kRinvWild = -1 for n outside [2^-40, 2^40], 0 for a row that takes no
part (hidden, behind its segment's last row, n < 2^-126).  A pair is CERTIFIED when both rinv are positive.

The slack (`slack`, `Model.rows`).  The device computes s = fl(fl(acc ra) rb) in f32 with acc the sum v_mfma_f32_32x32x16_bf16
leaves of the Dp products bf16(a_i) bf16(b_i), Dp / 16 instructions chained through the accumulator.
  - Every product of two 8-bit significands is exact in f32, so acc differs from the exact sum only by the additions.  Dp - 1
    additions in ANY order, each rounded in ANY direction (relative error below 2^-23), err by at most (Dp - 1) 2^-23 sum |a^_i b^_i|:
    below eps32(D) sum |a^_i b^_i| with eps32(D) = (Dp + 16) 1.2e-7, the bound the project claims for such a chain
    (searcher_pass.cpp fill_params, screens_ref.bf16_slack).  screens_ref bounds the sum of magnitudes by |a^||b^|; the model has the
    rows, so it takes T[a, b] = sum |a^_i b^_i| ra rb itself (T <= (1 + 2^-8)^2, some 0.64 for Gaussian rows): never looser.
  - The two multiplications by ra and rb: 2^-24 each, of |s| <= (1 + 2^-8)^2.  One ulp of each rinv (the device's f64 sqrt and
    division against numpy's, then the rounding to f32): 2^-23 each.  Together 3 * 2^-23 |s| (1 + 2^-22), which is 2^-22 |s| and
    1.2e-7 |s| more; |s| <= T, and eps32 T has (17 * 1.2e-7 + Dp * 8e-10) T to spare over (Dp - 1) 2^-23 T: seventeen times that.
So |s_device - S| <= E = eps32(D) T + 2^-22, and slack(D) = eps32(D) (1 + 2^-8)^2 + 2^-22 bounds every E.  Every bracket is interval
arithmetic on [S - E, S + E]: `lo` counts what is listed whatever the device's rounding did, `hi` what may be.  A threshold built
from device scores (neighbours, trees, the labels' carried bound) is an interval too, so a comparison against it moves by both.
Wild rows list every defined pair, rows with rinv == 0 list nothing; both add the same to lo and hi.

The same functions count for a SIMULATED screen (`Model(..., simulate=seed)`): S plus noise of E's size rounded to f32, a point
instead of an interval, optionally with one fault of FAULTS built in.  test_pairs_cpu.py uses it to show the brackets have teeth."""
import functools
from collections import namedtuple

import numpy as np

from duplicates_ref import bf16_rne, make_ids

F32 = np.float32
BLOCK = 32            # kBlockRows
WAVES = 8             # kScreenWaves
MAX_SPANS = 512       # kMaxNeighborSpans
CHUNK = 1024          # owners of one block of the score matrix
RD = 2.0 ** -23       # __double2float_rd of a threshold of magnitude below 2 moves it by less than this


class ModelError(AssertionError):
    """the model cannot decide (its pair list was cut too high for this input): a fault of the test's setup, never of the device"""


# ---- host mirrors ---------------------------------------------------------------------------------------------------------------------
def padded(D):
    return (D + 63) // 64 * 64


def tile_rows(D):
    """mfma_pass_queries(Dp): the rows of the LDS tile, 128 / 64 / 32 for Dp <= 576 / <= 1216 / above (0: no tile fits)"""
    for nt in (4, 2, 1):
        if nt * 32 * padded(D) * 2 <= 156 * 1024:
            return nt * 32
    return 0


def eps32(D):
    return (padded(D) + 16) * 1.2e-7


def slack(D):
    """the bound of |s_device - S| for any certified pair (the module docstring derives it)"""
    return eps32(D) * (1 + 2.0 ** -8) ** 2 + 2.0 ** -22


def margin(D, scale=1.0):
    """selfjoin_margin(Dp) in f32 arithmetic"""
    return float(F32(scale) * (F32(0.00783) + F32(1.02) * (F32(padded(D) + 16) * F32(1.2e-7)) + F32(1e-6)))


def f32_down(x):
    y = F32(x)
    return float(y) if float(y) <= x else float(np.nextafter(y, F32(-np.inf)))


def f32_up(x):
    y = F32(x)
    return float(y) if float(y) >= x else float(np.nextafter(y, F32(np.inf)))


def screen_threshold(threshold, D, scale=1.0):
    """find_duplicates: nextafterf((float)((double)threshold - (double)margin), -inf)"""
    t = F32(float(F32(threshold)) - margin(D, scale))
    return float(np.nextafter(t, F32(-np.inf)))


def density_thresholds(threshold, D, scale=1.0):
    """density_clusters: (lo, hi) = thr -+ margin from f64, rounded to f32 and one step outwards"""
    t, m = float(F32(threshold)), margin(D, scale)
    return float(np.nextafter(F32(t - m), F32(-np.inf))), float(np.nextafter(F32(t + m), F32(np.inf)))


def neighbor_sample(TB, k):
    """neighbor_sample (row_jobs.cpp) -> (stride, span_len, spans)"""
    stride = min(4, max(1, TB // max(64, 4 * k)))
    sampled = (TB + stride - 1) // stride
    want = min(sampled, min(MAX_SPANS, max(64, 8 * k)))
    span_len = (sampled + want - 1) // want
    return stride, span_len, (sampled + span_len - 1) // span_len


def linkage_stride(TB):
    """LinkRounds::open: the sample of the trees' bound pass"""
    return min(4, max(1, TB // 64))


def join_spans(TB):
    """the grid's second dimension in launch_selfjoin_screen: spans of kJoinSpanBlocks = 256 blocks"""
    return (TB + 255) // 256


def canonical_norm2(rows):
    r = np.ascontiguousarray(rows, dtype=F32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.cumsum(r * r, axis=1)[:, -1]


def rinv_of(n2, searchable):
    """selfjoin_prep_kernel's rinv for canonical norms n2 [n] (f64) -> f32 [n]"""
    out = np.zeros(n2.shape, dtype=F32)
    has = searchable & (n2 >= 2.0 ** -126) & (n2 < np.inf)
    cert = has & (n2 >= 2.0 ** -40) & (n2 <= 2.0 ** 40)
    out[has] = F32(-1.0)
    out[cert] = (1.0 / np.sqrt(n2[cert])).astype(F32)
    return out


# ---- the corpus as a launch sees it ---------------------------------------------------------------------------------------------------
class Corpus:
    """rows [n, D] f32 as stored.  sources: the rows of every selected source (index arrays, in the order of the global positions);
    the launch numbers them source after source and pads each source's last block (every segment but a source's last is whole
    blocks in the tests).  hidden: bool [n], rows no search could return."""

    def __init__(self, rows, sources=None, hidden=None):
        rows = np.ascontiguousarray(rows, dtype=F32)
        n, self.D = rows.shape
        sources = [np.arange(n)] if sources is None else [np.asarray(s, dtype=np.int64) for s in sources]
        src = []
        for idx in sources:
            src += [idx, np.full((-len(idx)) % BLOCK, -1, dtype=np.int64)]
        self.src = np.concatenate(src)  # launch row -> row, -1 behind a source's last row
        self.L = len(self.src)
        self.TB = self.L // BLOCK
        self.rows_selected = int((self.src >= 0).sum())
        real = self.src >= 0
        at = np.where(real, self.src, 0)
        hidden = np.zeros(n, dtype=bool) if hidden is None else np.asarray(hidden, dtype=bool)
        n2 = canonical_norm2(rows)
        self.rinv = np.where(real, rinv_of(n2, ~hidden)[at], F32(0)).astype(F32)
        self.searchable = real & ~hidden[at]
        self.cert, self.part = self.rinv > 0, self.rinv != 0
        self.wild = self.part & ~self.cert
        self.P = int(self.part.sum())
        self.B = np.where(real[:, None], bf16_rne(rows).astype(np.float64)[at], 0.0)  # what the tile and the stream hold
        self.absB = np.abs(self.B)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            U = rows.astype(np.float64) / np.sqrt(n2)[:, None]
        self.U = np.where(self.part[:, None], U[at], 0.0)  # unit rows: the exact cosine of the trees' f64 step, up to 1e-16
        self.r64 = np.where(self.cert, self.rinv, 0).astype(np.float64)
        self.Br, self.absBr = self.B * self.r64[:, None], self.absB * self.r64[:, None]  # (the products with rinv: exact to 2^-53)
        self.tile = tile_rows(self.D)


FAULTS = ("shift", "rb_next", "stale_acc")  # faults of the score itself; the faults of a rule are arguments of the screen functions


class Model:
    """The scores of a corpus as intervals [S - E, S + E] (simulate=None) or as one simulated device's f32 scores (simulate=seed,
    fault: one of FAULTS or None).  rows(a0, a1) -> (Slo, Shi) [a1 - a0, L], NaN where the pair is not certified."""

    def __init__(self, corpus, simulate=None, fault=None):
        assert fault is None or (fault in FAULTS and simulate is not None)
        self.c = corpus
        self.simulate, self.fault = simulate, fault
        self._dense = None
        self._pairs = {}

    def _finish(self, S, T, rows_rinv, cols_rinv, seed, unit=1.0):
        """S, T [r, c] exact score and magnitude sum; rinv of the rows / columns (f64, 0 where not certified)"""
        T *= eps32(self.c.D)  # (in place: the blocks of a large corpus are 100 MB each)
        T += 2.0 ** -22 * unit
        E = T
        if self.simulate is None:
            lo = S - E
            S += E
            hi = S
        else:
            rng = np.random.default_rng([self.simulate, seed])
            s = S + E * rng.uniform(-1.0, 1.0, size=S.shape)
            if self.fault == "shift":
                s = s + 1e-3
            lo = s.astype(F32).astype(np.float64)
            hi = lo.copy()
        for X in (lo, hi):
            X[~(rows_rinv > 0), :] = np.nan
            X[:, ~(cols_rinv > 0)] = np.nan
        return lo, hi

    def rows(self, a0, a1):
        c = self.c
        if self._dense is not None:
            return self._dense[0][a0:a1], self._dense[1][a0:a1]
        r = c.r64
        S = c.Br[a0:a1] @ c.Br.T
        T = c.absBr[a0:a1] @ c.absBr.T
        if self.fault == "rb_next":  # the rinv of block g + 1 beside the accumulators of block g
            nxt = np.concatenate([r[BLOCK:], r[-BLOCK:]])
            with np.errstate(invalid="ignore", divide="ignore"):
                S = np.where(r[None, :] > 0, S * (nxt / r)[None, :], S)
        if self.fault == "stale_acc":  # block g starts from the sum of block g - 8, the wave's block before it
            back = WAVES * BLOCK
            with np.errstate(invalid="ignore", divide="ignore"):
                carry = S[:, :-back] * (r[back:] / r[:-back])[None, :]
            S = S.copy()
            S[:, back:] += np.where(np.isfinite(carry), carry, 0.0)
        return self._finish(S, T, r[a0:a1], r, a0)

    def dense(self):
        """keep the whole square (small corpora: every screen of a case reads it)"""
        if self._dense is None:
            parts = [self.rows(a0, min(self.c.L, a0 + CHUNK)) for a0 in range(0, self.c.L, CHUNK)]
            self._dense = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        return self

    def chunks(self):
        for a0 in range(0, self.c.L, CHUNK):
            a1 = min(self.c.L, a0 + CHUNK)
            yield (a0, a1) + self.rows(a0, a1)


def _undecided(c, a0, a1):
    """[a1 - a0, L]: pairs of participating rows that are not certified — a wild row: every such pair is listed"""
    out = np.zeros((a1 - a0, c.L), dtype=bool)
    if c.wild.any():
        out = (c.part[a0:a1, None] & c.part[None, :]) & ~(c.cert[a0:a1, None] & c.cert[None, :])
    return out


# ---- join -----------------------------------------------------------------------------------------------------------------------------
def join(m, threshold, margin_scale=1.0, diagonal=True):
    """selfjoin_screen_kernel / JoinPolicy: s >= screen_threshold, each unordered pair once: the blocks at and behind the tile's
    first, and inside the tile's own blocks only row a before row b.  diagonal=False: that last rule dropped."""
    c = m.c
    thr = screen_threshold(threshold, c.D, margin_scale)
    col = np.arange(c.L)
    lo = hi = 0
    for a0, a1, Slo, Shi in m.chunks():
        row = np.arange(a0, a1)
        first = row if diagonal else row // c.tile * c.tile - 1  # (the tile's own rows again, the row itself included)
        mask = col[None, :] > first[:, None]
        wild = int((_undecided(c, a0, a1) & mask).sum())
        lo += int(((Slo >= thr) & mask).sum()) + wild
        hi += int(((Shi >= thr) & mask).sum()) + wild
    return lo, hi


# ---- density --------------------------------------------------------------------------------------------------------------------------
def density(m, threshold, margin_scale=1.0, diagonal=True):
    """density_screen_kernel<NT, false>: s >= hi a sure pair, lo <= s < hi (or a wild row) a band pair, each unordered pair once
    -> {"sure_pairs": (lo, hi), "candidates": (lo, hi)}"""
    c = m.c
    t_lo, t_hi = density_thresholds(threshold, c.D, margin_scale)
    col = np.arange(c.L)
    sure, band = [0, 0], [0, 0]
    for a0, a1, Slo, Shi in m.chunks():
        row = np.arange(a0, a1)
        first = row if diagonal else row // c.tile * c.tile - 1
        mask = col[None, :] > first[:, None]
        wild = int((_undecided(c, a0, a1) & mask).sum())
        sure[0] += int(((Slo >= t_hi) & mask).sum())
        sure[1] += int(((Shi >= t_hi) & mask).sum())
        band[0] += int(((Slo >= t_lo) & (Shi < t_hi) & mask).sum()) + wild
        band[1] += int(((Shi >= t_lo) & (Slo < t_hi) & mask).sum()) + wild
    return {"sure_pairs": tuple(sure), "candidates": tuple(band)}


# ---- assign ---------------------------------------------------------------------------------------------------------------------------
def label_constants(labels, metric, D, margin_scale=1.0):
    """(w, mg, wr) per label as assign_labels_kernel writes them (f32 values, as f64), wr the factor of the exact score"""
    labels = np.ascontiguousarray(labels, dtype=F32)
    n2 = canonical_norm2(labels)
    rinv = rinv_of(n2, np.ones(len(labels), dtype=bool))
    mg0 = F32(margin(D, margin_scale))
    w, mg = rinv.astype(np.float64), np.full(len(labels), float(mg0))
    if metric == "dot":
        w = np.where((rinv > 0) | (n2 == 0.0), 1.0, -1.0)
        mg = np.array([f32_up(float(mg0) * np.sqrt(x) * (1.0 + 2.0 ** -40)) for x in n2])
    return w, mg, np.where(w > 0, w, 0.0), np.sqrt(n2)


def assign(m, labels, metric="cosine", margin_scale=1.0, carry=True):
    """assign_screen_kernel / AssignPolicy, one launch per tile of tile_rows(D) labels, in order: s = acc rinv_row w; the row's bound
    is the largest s - mg over the labels of the tiles so far (this one included); (row, label) is listed iff s + mg >= the bound.
    The bound is a device score: it moves by the slack too.  carry=False: every tile starts from -inf.
    E here: eps32 T + 2^-21 |l| under dot (w = 1: the scores are in units of |l|), of 1 under cosine — the 2^-22 of the row-pair
    score and one rounding each in s - mg and s + mg."""
    c = m.c
    labels = np.ascontiguousarray(labels, dtype=F32)
    K = len(labels)
    w, mg, wr, norm = label_constants(labels, metric, c.D, margin_scale)
    rinv = c.rinv.astype(np.float64)
    if metric == "dot":  # assign_begin_kernel: a searchable row without a cosine is wild under dot
        rinv = np.where((c.rinv == 0) & c.searchable, -1.0, rinv)
    rr = np.where(rinv > 0, rinv, 0.0)
    LB = bf16_rne(labels).astype(np.float64)
    S = (c.B @ LB.T) * rr[:, None] * wr[None, :]
    T = (c.absB @ np.abs(LB).T) * rr[:, None] * wr[None, :]
    unit = (norm if metric == "dot" else np.ones(K))[None, :]
    if m.fault == "rb_next":
        nxt = np.concatenate([rr[BLOCK:], rr[-BLOCK:]])
        with np.errstate(invalid="ignore", divide="ignore"):
            S = np.where(rr[:, None] > 0, S * (nxt / rr)[:, None], S)
    Slo, Shi = m._finish(S, T, rr, wr, 1 << 20, unit=2.0 * unit)
    tl = c.tile
    b_hi = np.full(c.L, -np.inf)
    b_lo = np.full(c.L, -np.inf)
    lo = hi = 0
    for j0 in range(0, K, tl):
        j = slice(j0, min(K, j0 + tl))
        ok = ~np.isnan(Slo[:, j])
        up = np.where(ok, Shi[:, j] - mg[None, j], -np.inf).max(axis=1)
        dn = np.where(ok, Slo[:, j] - mg[None, j], -np.inf).max(axis=1)
        b_hi, b_lo = (np.maximum(b_hi, up), np.maximum(b_lo, dn)) if carry else (up, dn)
        wild = int(((rinv != 0)[:, None] & (w[None, j] != 0) & ~ok).sum())
        with np.errstate(invalid="ignore"):
            lo += int((ok & (Slo[:, j] + mg[None, j] >= b_hi[:, None])).sum()) + wild
            hi += int((ok & (Shi[:, j] + mg[None, j] >= b_lo[:, None])).sum()) + wild
    return lo, hi


# ---- neighbours -----------------------------------------------------------------------------------------------------------------------
def neighbors(m, k, margin_scale=1.0, margins=2.0):
    """neighbors_screen_kernel: the bound pass leaves per owner and span the largest certified s over the sampled blocks (the owner
    itself and uncertified partners left out); thr = (k-th largest span maximum) - 2 margin, rounded down, -inf with fewer than k;
    the list pass keeps the directed pairs a != b with s >= thr[a] over all blocks.  margins: the factor in the place of 2."""
    c = m.c
    stride, span_len, spans = neighbor_sample(c.TB, k)
    per = stride * span_len * BLOCK
    col = np.arange(c.L)
    samp = col[(col // BLOCK) % stride == 0]
    starts = np.searchsorted(samp // per, np.arange(spans))
    mg = margin(c.D, margin_scale)
    lo = hi = 0
    for a0, a1, Slo, Shi in m.chunks():
        row = np.arange(a0, a1)
        own = col[None, :] == row[:, None]
        with np.errstate(invalid="ignore"):
            kth = []
            for X in (Slo, Shi):
                X = np.where(own | np.isnan(X), -np.inf, X)
                mx = np.maximum.reduceat(X[:, samp], starts, axis=1)
                kth.append(np.partition(mx, spans - k, axis=1)[:, spans - k] if spans >= k else np.full(a1 - a0, -np.inf))
            thr_lo = kth[0] - margins * mg - RD
            thr_hi = kth[1] - margins * mg
            wild = int((_undecided(c, a0, a1) & ~own).sum())
            lo += int(((Slo >= thr_hi[:, None]) & ~own).sum()) + wild
            hi += int(((Shi >= thr_lo[:, None]) & ~own).sum()) + wild
    return lo, hi


# ---- the trees ------------------------------------------------------------------------------------------------------------------------
Pairs = namedtuple("Pairs", "ia ib slo shi c floor")


def pair_list(m, budget=500000):
    """Every unordered pair of participating rows (launch rows ia < ib) with its score interval (NaN: not certified) and its exact
    cosine c — or, for a corpus with more than `budget` pairs, those whose c or upper score reaches `floor`, the level above
    which about `budget` pairs lie.  The rounds check at every use that nothing below the floor could have mattered."""
    if budget in m._pairs:
        return m._pairs[budget]
    c = m.c
    total = c.P * (c.P - 1) // 2
    floor = -np.inf
    col = np.arange(c.L)
    out = []
    for a0, a1, Slo, Shi in m.chunks():
        C = c.U[a0:a1] @ c.U.T
        both = (c.part[a0:a1, None] & c.part[None, :]) & (col[None, :] > np.arange(a0, a1)[:, None])
        V = np.where(np.isnan(Shi), C, np.maximum(Shi, C))
        if a0 == 0 and total > budget:
            floor = float(np.quantile(V[both], 1.0 - budget / total))
        keep = both & ((V >= floor) | np.isnan(Shi))
        ia, ib = np.nonzero(keep)
        out.append((ia + a0, ib, Slo[ia, ib], Shi[ia, ib], C[ia, ib]))
    p = Pairs(*(np.concatenate([o[i] for o in out]) for i in range(5)), floor)
    m._pairs[budget] = p
    return p


def cores_of(c, p, j):
    """the j-th largest exact cosine of every participating row with another one, from the pair list -> [L] (+inf for j = 0)"""
    core = np.full(c.L, np.nan)
    if j <= 0:
        core[c.part] = np.inf
        return core
    row = np.concatenate([p.ia, p.ib])
    val = np.concatenate([p.c, p.c])
    order = np.lexsort((-val, row))
    row, val = row[order], val[order]
    first = np.searchsorted(row, np.arange(c.L))
    count = np.searchsorted(row, np.arange(c.L), side="right") - first
    live = np.nonzero(c.part)[0]
    if (count[live] < j).any():
        raise ModelError("a row has fewer than %d pairs above the floor %g" % (j, p.floor))
    core[live] = val[first[live] + j - 1]
    if (core[live] < p.floor).any():
        raise ModelError("a core lies below the floor %g" % p.floor)
    return core


def _group_max(keys, n, *vals):
    """the maximum of every array of `vals` per key -> one [n] array each, -inf where a key does not occur"""
    outs = [np.full(n, -np.inf) for _ in vals]
    if len(keys):
        order = np.argsort(keys, kind="stable")
        k = keys[order]
        starts = np.nonzero(np.concatenate([[True], k[1:] != k[:-1]]))[0]
        for out, v in zip(outs, vals):
            out[k[starts]] = np.maximum.reduceat(v[order], starts)
    return outs


Round = namedtuple("Round", "before after lo hi bound_repeated")
Tree = namedtuple("Tree", "rounds edges")  # edges: (pos_a, pos_b) of the exact tree, positions among the selected rows, unordered


def tree_rounds(m, min_items=None, margin_scale=1.0, margins=2.0, cap_list=True, budget=500000):
    """The Borůvka rounds of linkage_tree (min_items=None) and reach_tree (LinkRounds::run, LinkPolicy) -> Tree.
    The exact side: every component takes its best outgoing edge in the strict order (w descending, lower row, higher row), w the
    exact cosine, capped by the two cores for the reach tree; the chosen edges merge.  The screen of a round, with the components
    before it: comp_max = the largest certified s (reach: min(s, klo_a, klo_b)) over owners of the component and certified partners
    of another one in the sampled blocks (every stride-th, stride = linkage_stride(TB); once more at stride 1 when a certified
    component found no bound and there are two certified components); thr = comp_max - 2 margin, rounded down; candidates: the
    directed pairs of different components with s >= thr[comp[a]] (or a wild row) and, reach, khi_a >= thr and khi_b >= thr.
    cap_list=False: those two tests dropped.  margins: the factor in the place of 2."""
    c = m.c
    p = pair_list(m, budget)
    mg = margin(c.D, margin_scale)
    reach = min_items is not None
    w = p.c
    klo = khi = None
    if reach:
        core = cores_of(c, p, min(int(min_items) - 1, c.P - 1))
        w = np.minimum(np.minimum(core[p.ia], core[p.ib]), p.c)
        with np.errstate(invalid="ignore"):
            klo = np.array([f32_down(x) if x == x else -np.inf for x in core])
            khi = np.array([f32_up(x) if x == x else -np.inf for x in core])
    order = np.lexsort((p.ib, p.ia, -w))
    ia, ib, slo, shi, w = p.ia[order], p.ib[order], p.slo[order], p.shi[order], w[order]
    comp = np.arange(c.L)
    stride0 = linkage_stride(c.TB)
    rounds, edges = [], []
    ncomp = c.P
    while ncomp > 1:
        ca, cb = comp[ia], comp[ib]
        f = ca != cb
        ia, ib, slo, shi, w, ca, cb = ia[f], ib[f], slo[f], shi[f], w[f], ca[f], cb[f]
        n = len(ia)
        roots = np.unique(comp[c.part])
        # the exact choice: the first pair of each component in the edge order
        idx = np.arange(n)
        first = np.full(c.L, n)
        first[cb[::-1]] = idx[::-1]
        f2 = np.full(c.L, n)
        f2[ca[::-1]] = idx[::-1]
        first = np.minimum(first, f2)
        if (first[roots] >= n).any() or (w[first[roots]] < p.floor).any():
            raise ModelError("a component's best edge lies below the floor %g" % p.floor)
        # the bound
        ok = ~np.isnan(slo)
        vlo, vhi = slo, shi
        if reach:
            cap = np.minimum(klo[ia], klo[ib])
            vlo, vhi = np.minimum(slo, cap), np.minimum(shi, cap)
        cert_roots = np.unique(comp[c.cert])

        def bound(stride):
            sa, sb = ok & ((ia // BLOCK) % stride == 0), ok & ((ib // BLOCK) % stride == 0)
            keys = np.concatenate([ca[sb], cb[sa]])
            mlo, mhi = _group_max(keys, c.L, np.concatenate([vlo[sb], vlo[sa]]), np.concatenate([vhi[sb], vhi[sa]]))
            # which certified components have a certified foreign row in the sample at all
            srow = c.cert & ((np.arange(c.L) // BLOCK) % stride == 0)
            in_comp = np.bincount(comp[srow], minlength=c.L)
            has = (int(srow.sum()) - in_comp) > 0
            if (has[cert_roots] & (mlo[cert_roots] < p.floor)).any():
                raise ModelError("a component's bound lies below the floor %g" % p.floor)
            return mlo, mhi, cert_roots[~has[cert_roots]]

        mlo, mhi, unbounded = bound(stride0)
        repeated = stride0 > 1 and len(unbounded) > 0 and len(cert_roots) >= 2
        if repeated:
            mlo, mhi, unbounded = bound(1)
        thr_lo = mlo - margins * mg - RD
        thr_hi = mhi - margins * mg
        finite = np.isfinite(thr_lo[cert_roots])
        if finite.any() and thr_lo[cert_roots][finite].min() < p.floor:
            raise ModelError("a threshold lies below the floor %g" % p.floor)
        # the list: both directions of every foreign pair
        lo = hi = 0
        with np.errstate(invalid="ignore"):
            for own, oth, co in ((ia, ib, ca), (ib, ia, cb)):
                t_lo, t_hi = thr_lo[co], thr_hi[co]
                pl = np.where(ok, slo >= t_hi, True)
                ph = np.where(ok, shi >= t_lo, True)
                if reach and cap_list:
                    pl &= (khi[own] >= t_hi) & (khi[oth] >= t_hi)
                    ph &= (khi[own] >= t_lo) & (khi[oth] >= t_lo)
                lo += int(pl.sum())
                hi += int(ph.sum())
        # the merge
        parent = {int(r): int(r) for r in roots}

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for e in np.unique(first[roots]).tolist():
            edges.append((int(ia[e]), int(ib[e])))
            x, y = find(int(ca[e])), find(int(cb[e]))
            if x != y:
                parent[max(x, y)] = min(x, y)
        relabel = np.arange(c.L)
        for r in roots.tolist():
            relabel[r] = find(r)
        comp = relabel[comp]
        after = len(np.unique(comp[c.part]))
        rounds.append(Round(ncomp, after, lo, hi, bool(repeated)))
        assert after <= ncomp // 2
        ncomp = after
    out = np.cumsum(c.src >= 0) - 1  # launch row -> position among the selected rows
    e = np.array(edges, dtype=np.int64).reshape(-1, 2)
    return Tree(rounds, (out[e[:, 0]], out[e[:, 1]]))


def total(tree):
    return sum(r.lo for r in tree.rounds), sum(r.hi for r in tree.rounds)


# ---- the cases test_pairs_cpu.py and test_pairs_gpu.py share ---------------------------------------------------------------------------
# A corpus: rows, ids, the pieces it is added in [(source id, first row, end row)] (each announced, so that it gets a segment of its
# own; a piece that is not a whole number of blocks is filled by its source's next one: a source's rows are contiguous in the launch
# and only its last block is padded), and the rows to hide.
Made = namedtuple("Made", "rows ids pieces hidden")
N_BASE = 3007  # 94 blocks, a last block of 31 rows, a partial last tile at every tile size
SEG_SIZES = [64, 96, 32, 1, 128, 5, 300, 2381]
SEG_SOURCE = [1, 2, 3, 1, 2, 3, 2, 1]  # source 1: 64, 1 + 31, 2350 rows;  2: 96, 128, 300;  3: 32, 5 — eight segments


def _gaussian(n, dim, seed):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(F32)


def _shared(n, dim, seed, rank=16):
    """Gaussian rows plus a component from a space of `rank` dimensions that all share: the scores spread over +-0.3 instead of
    +-0.03 at 1280-d, and fewer of the pairs a threshold keeps lie within the slack of it"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)) + rng.standard_normal((n, rank)) @ rng.standard_normal((rank, dim)) / np.sqrt(rank)
    return x.astype(F32)


def _clump(n, dim, seed, members=600, cos=0.95):
    """Gaussian rows, `members` of them (anywhere) at cosine `cos` of one centre: some members^2 / 2 pairs near cos^2"""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, dim))
    centre = rng.standard_normal(dim)
    centre /= np.linalg.norm(centre)
    for r in rng.permutation(n)[:members]:
        u = rng.standard_normal(dim)
        u -= (u @ centre) * centre
        rows[r] = np.sqrt(dim) * (cos * centre + np.sqrt(1 - cos * cos) * u / np.linalg.norm(u))
    return rows.astype(F32)


def _odd(n, dim, seed):
    """a zero row, a hidden block and four wild rows: two of |x| ~ 2^-33, two of 2^28 (|x|^2 outside [2^-40, 2^40])"""
    rows = _gaussian(n, dim, seed)
    rows[77] = 0.0
    scale = 2.0 ** -np.ceil(np.log2(np.sqrt(dim)))
    for r, e in ((5, -33), (1500, -33), (2000, 28), (3006, 28)):
        rows[r] = np.ldexp(rows[r] * F32(scale), e)
    hidden = np.zeros(n, dtype=bool)
    hidden[40 * BLOCK : 41 * BLOCK] = True
    return rows, hidden


def _make(key):
    kind, dim = key.rstrip("0123456789"), int(key[len(key.rstrip("0123456789")):])
    pieces, hidden = None, None
    if kind == "g":
        rows = _gaussian(N_BASE, dim, dim)
    elif kind == "s":
        rows = _shared(N_BASE, dim, dim)
    elif kind == "big":
        rows = _gaussian(12320, dim, 7)
    elif kind == "clump":
        rows = _clump(N_BASE, dim, 11)
    elif kind == "odd":
        rows, hidden = _odd(N_BASE, dim, 13)
    elif kind == "seg":
        rows = _gaussian(N_BASE, dim, 17)
        first = np.concatenate([[0], np.cumsum(SEG_SIZES)])
        pieces = [(sid, int(first[i]), int(first[i + 1])) for i, sid in enumerate(SEG_SOURCE)]
    else:
        raise KeyError(key)
    n = rows.shape[0]
    ids = make_ids(np.random.default_rng(n + dim), n)
    return Made(np.ascontiguousarray(rows), ids, pieces or [(1, 0, n)], np.zeros(n, dtype=bool) if hidden is None else hidden)


@functools.lru_cache(maxsize=4)
def made(key):
    return _make(key)


def selected(md, select=None):
    """the rows of each selected source (None: all), in the order of the global positions: by source as created, then as added"""
    order = []
    for sid, _lo, _hi in md.pieces:
        if sid not in order:
            order.append(sid)
    return [np.concatenate([np.arange(lo, hi) for s, lo, hi in md.pieces if s == sid]) for sid in order if select is None or sid in select]


@functools.lru_cache(maxsize=2)
def model(key, select=None):
    md = made(key)
    m = Model(Corpus(md.rows, selected(md, select), md.hidden))
    return m.dense() if m.c.L <= 4096 else m


def labels_for(key, K, metric, alike=False):
    """K label vectors for a corpus: Gaussian (alike: all at cosine 0.9995 of one vector); under dot, lengths spread over [0.5, 2]
    times the Gaussian one"""
    dim = made(key).rows.shape[1]
    rng = np.random.default_rng([K, dim, 5])
    lab = rng.standard_normal((K, dim))
    if alike:
        centre = rng.standard_normal(dim)
        lab = 0.9995 * centre[None, :] + np.sqrt(1 - 0.9995 ** 2) * lab * np.linalg.norm(centre) / np.linalg.norm(lab, axis=1)[:, None]
    if metric == "dot":
        lab = lab * rng.uniform(0.5, 2.0, size=(K, 1))
    return np.ascontiguousarray(lab, dtype=F32)


# A run: one call on one corpus.  cap: the width (hi - lo) / lo the bracket of the model may have (test_pairs_cpu.py): 0.02 for the
# fixed-threshold screens at Dp <= 768 (join, density, one-tile assign), 0.05 for wider rows and for the screens whose threshold
# comes from device scores.  select: the source list of the call (None: every source).  grows: the list outgrows its first capacity.
Run = namedtuple("Run", "key screen args cap select grows", defaults=(None, False))


def _z(dim, z):
    return float(F32(z / np.sqrt(dim)))


def _runs():
    runs = []
    base = {64: "g64", 128: "g128", 384: "g384", 576: "g576", 640: "g640", 1280: "s1280"}
    for dim, key in base.items():
        fixed = 0.02 if dim <= 768 else 0.05
        t1, t2 = (_z(dim, 3.0), _z(dim, 3.3)) if key[0] == "g" else (0.30, 0.38)
        runs.append(Run(key, "join", (t2,), fixed))
        runs += [Run(key, "density", (t, 4), fixed) for t in (t1, t2)]
    for dim in (64, 384, 640, 1280):
        key = base[dim]
        for metric in ("cosine", "dot"):
            runs.append(Run(key, "assign", (100, metric), 0.02 if dim <= 576 else 0.05))
        runs.append(Run(key, "neighbors", (10,), 0.05))
        runs.append(Run(key, "linkage", (), 0.05))
        runs.append(Run(key, "reach", (5,), 0.05))
    runs += [Run("g384", "neighbors", (k,), 0.05) for k in (1, 64)]
    runs += [Run("g384", "reach", (mi,), 0.05) for mi in (2, 16)]
    runs += [Run(key, "assign", (300, metric), 0.05) for key in ("g384", "g640") for metric in ("cosine", "dot")]
    # more than one span, a sampled bound pass
    runs += [Run("big64", "join", (_z(64, 4.0),), 0.02), Run("big64", "neighbors", (10,), 0.05), Run("big64", "linkage", (), 0.05)]
    # eight segments in three sources: whole, the source list in another order, two of the three
    for select in (None, (3, 1, 2), (3, 1)):
        runs += [Run("seg384", "join", (_z(384, 3.3),), 0.02, select), Run("seg384", "neighbors", (10,), 0.05, select)]
    runs += [Run("seg384", "density", (_z(384, 3.0), 4), 0.02, None), Run("seg384", "linkage", (), 0.05, (3, 1)), Run("seg384", "assign", (100, "cosine"), 0.02, (3, 1))]
    # rows that take no part and wild rows
    runs += [Run("odd384", "join", (_z(384, 3.3),), 0.02), Run("odd384", "density", (_z(384, 3.0), 4), 0.02), Run("odd384", "neighbors", (10,), 0.05),
             Run("odd384", "assign", (100, "cosine"), 0.02), Run("odd384", "assign", (100, "dot"), 0.02), Run("odd384", "linkage", (), 0.05),
             Run("odd384", "reach", (5,), 0.05)]
    # lists that outgrow their first capacity
    runs += [Run("clump384", "join", (0.75,), 0.02, None, True), Run("clump384", "density", (0.8945, 4), 0.02, None, True),
             Run("clump384", "neighbors", (1,), 0.05, None, True), Run("g384", "assign", (300, "alike"), 0.05, None, True),
             Run("clump384", "linkage", (), 0.05, None, True), Run("clump384", "reach", (5,), 0.05, None, True)]
    return sorted(runs, key=lambda r: (r.key, r.select or ()))  # (a corpus's runs together: its model is built once)


RUNS = _runs()


def run_id(r):
    return "-".join([r.key, r.screen] + [str(a) for a in r.args] + (["src" + "".join(map(str, r.select))] if r.select else []))


def first_capacity(r, c):
    """the room of the candidate list before any rerun (row_jobs.cpp); the trees': per round"""
    rows, nr = c.rows_selected, c.L
    if r.screen in ("join", "density"):
        return max(65536, 2 * rows)
    if r.screen == "assign":
        return max(65536, 4 * rows)
    if r.screen == "neighbors":
        return max(65536, 32 * r.args[0] * rows)
    return max(65536, 32 * nr)


def assign_labels(r):
    K, metric = r.args
    return (labels_for(r.key, K, "cosine", alike=True), "cosine") if metric == "alike" else (labels_for(r.key, K, metric), metric)


def bracket(r, m=None, **fault):
    """What the model says of run r -> join, assign, neighbors: (lo, hi); density: {"sure_pairs": (lo, hi), "candidates": (lo, hi)};
    linkage: Tree; reach: (the core step's (lo, hi), Tree).  m: another Model of the run's corpus (a simulated device); fault: the
    arguments that build a fault into the rule"""
    m = model(r.key, r.select) if m is None else m
    if r.screen == "join":
        return join(m, r.args[0], **fault)
    if r.screen == "density":
        return density(m, r.args[0], **fault)
    if r.screen == "assign":
        lab, metric = assign_labels(r)
        return assign(m, lab, metric, **fault)
    if r.screen == "neighbors":
        return neighbors(m, r.args[0], **fault)
    if r.screen == "linkage":
        return tree_rounds(m, **fault)
    j = min(r.args[0] - 1, m.c.P - 1)
    core_fault = {k: v for k, v in fault.items() if k != "cap_list"}
    return (neighbors(m, j, **core_fault) if j >= 1 else (0, 0)), tree_rounds(m, r.args[0], **fault)


def brackets_of(r, b):
    """every (name, lo, hi) of a bracket() result; the trees: the sum over the rounds first, then every round"""
    if r.screen == "density":
        return [(k, v[0], v[1]) for k, v in b.items()]
    if r.screen in ("linkage", "reach"):
        core, tree = b if r.screen == "reach" else (None, b)
        out = [("core_candidates",) + tuple(core)] if core is not None else []
        return out + [("candidates",) + total(tree)] + [("round %d" % i, x.lo, x.hi) for i, x in enumerate(tree.rounds)]
    return [("candidates", b[0], b[1])]
