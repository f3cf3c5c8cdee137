"""A float64 numpy model of the threshold a TOP-K pass starts from, written from prep_seed_kernel / prep_seed_mfma_kernel,
seed_threshold_key / is_seed_block, set_guess and launch_prep_seed (csrc/scan_kernels.hip) and from fill_params / choose_guess
(csrc/searcher_pass.cpp), on top of the screens' model of tests/screens_ref.py.  TEST INFRASTRUCTURE ONLY:
tests/test_seed_cpu.py checks the planted corpora below against the conditions the GPU test rests on, tests/test_seed_gpu.py
holds the device's survivor counts of top-k passes against the model.

  seed_plan    (seed_blocks, seed_shift) of a pass whose first segment has seg0_rows rows (fill_params)
  seed_form    which seed kernel launch_prep_seed takes: "mfma" | "valu1" | "valu8" | "valu16"
  seed_sample  the sample: position sr = 32 (sample block) + (row in block)  ->  row of segment 0
  seed_slots   slot j of every query: the best score over the seed rows with sr % k == j
  guess_rank   the spec_rank choose_guess picks;  tau_start: the threshold the scan starts from
  Pinned       a planted corpus whose k best rows per query are seed rows, one in each group: tau is constant over the pass
  Guess        a planted corpus whose k best rows lie outside the seed blocks: the guess holds

Brackets.  A slot holds an f32 FMA-chain score of a row (the MFMA seed's v_mfma_f32_32x32x2_f32 is such a chain): it lies within
e = eps32(D) unit of the float64 score, the bound screens_ref.fine_slack takes for such a chain.  The screens' models are
therefore evaluated at tau + e, tightened by their own slack, for the low end and at tau - e, loosened by it, for the high end."""
from collections import namedtuple

import numpy as np

import screens_ref as sr
from screens_ref import Queries, Rows, eps32, keep_bf16, keep_fine, keep_int8, keep_mid, margins, scan_form  # noqa: F401

BLOCK_ROWS, SEED_PART_ROWS, SEED_PARTS, MAX_K = 32, 256, 64, 128       # scan.h: kBlockRows, kSeedPartRows, kSeedParts, kMaxK
FLAG_SEED16, FLAG_VALU_SEED, FLAG_NO_GUESS, FLAG_NO_LEARNED = 1 << 1, 1 << 2, 1 << 5, 1 << 7  # scan.h
LDS_ROOM = sr.LDS_ROOM


def with_parts(parts):
    """the seed-parts field of the tuning word (scan.h: flags_seed_parts, bits 16..23)"""
    assert 0 <= parts <= 0xFF
    return parts << 16


# ---- the launch side --------------------------------------------------------------------------------------------------------------------
def seed_plan(seg0_rows, flags):
    """fill_params: `p.seed_blocks = min(min(seed_parts, kSeedParts) * kSeedPartRows / kBlockRows, seg0_blocks)`, then the largest
    stride 2^shift with seed_blocks << shift <= seg0_blocks"""
    parts = ((flags >> 16) & 0xFF) or SEED_PARTS
    seg0_blocks = (seg0_rows + BLOCK_ROWS - 1) // BLOCK_ROWS
    blocks = min(min(parts, SEED_PARTS) * SEED_PART_ROWS // BLOCK_ROWS, seg0_blocks)
    shift = 0
    while (blocks << (shift + 1)) <= seg0_blocks and shift < 20:
        shift += 1
    return blocks, shift


def seed_form(B, Dp, k, flags):
    """launch_prep_seed, branch by branch"""
    lds1 = Dp * 4 + MAX_K * 4
    lds_mfma = 32 * (Dp + 4) * 4 + 32 * k * 4
    if lds_mfma <= LDS_ROOM and not flags & FLAG_VALU_SEED:
        return "mfma"
    if B <= 2 or 8 * lds1 > 64 * 1024:
        return "valu1"
    if B <= 32 or 16 * lds1 > 64 * 1024 or not flags & FLAG_SEED16:
        return "valu8"
    return "valu16"


def seed_sample(seg0_rows, plan):
    """(sr, row): the positions in the sample that hold a row, and that row of segment 0 — row sr & 31 of block
    (sr >> 5) << seed_shift, as both seed kernels index it and is_seed_block tells it"""
    blocks, shift = plan
    sample = np.arange(blocks * BLOCK_ROWS, dtype=np.int64)
    row = (((sample >> 5) << shift) << 5) | (sample & 31)
    ok = row < seg0_rows
    return sample[ok], row[ok]


def scores64(rows, qs):
    """the float64 score of every (row, query), the product keep_fine compares; NaN / inf where the row has none"""
    return sr._memo(rows, qs, "s32", lambda: (rows.x @ qs.qp.T) * rows.scale.astype(np.float64)[:, None])


def seed_slots(rows, qs, k, plan, drop=None, move=None):
    """[B, k] float64: slot j = the best score over the seed rows of `rows` (the pass's first segment) with sr % k == j that have
    a scale and a finite score; -inf for a group without one.  The two faults test_seed_cpu.py plants:
      drop [B]                  one row per query that the seed does not see
      move ([B] row, [B] group) one row per query that is ranked in another group than its own"""
    sample, row = seed_sample(rows.n, plan)
    s = scores64(rows, qs)[row]                                          # [seed rows, B]
    s = np.where((rows.scale[row] != 0)[:, None] & np.isfinite(s), s, -np.inf)
    slots = np.full((qs.B, k), -np.inf)
    if drop is None and move is None:
        for j in range(k):                                               # (every query has the same groups)
            slots[:, j] = s[sample % k == j].max(axis=0, initial=-np.inf)
        return slots
    group = np.broadcast_to((sample % k)[:, None], s.shape).copy()
    at = {int(r): i for i, r in enumerate(row)}
    if drop is not None:
        for q, r in enumerate(drop):
            s[at[int(r)], q] = -np.inf
    if move is not None:
        for q, (r, g) in enumerate(zip(*move)):
            group[at[int(r)], q] = g
    for j in range(k):
        slots[:, j] = np.where(group == j, s, -np.inf).max(axis=0, initial=-np.inf)
    return slots


def guess_rank(k, rows, seed_rows):
    """choose_guess: the smallest j < k with C(k - 1, j) ratio^j < 1e-6, ratio = seed rows / rows; None: no guess"""
    ratio = seed_rows / max(rows, 1)
    binom = rj = 1.0
    for j in range(1, k):
        if not ratio < 0.25:
            break
        binom *= (k - j) / j
        rj *= ratio
        if binom * rj < 1e-6:
            return j
    return None


def tau_start(slots, rank):
    """[B]: what every consumer of a threshold starts from, max(seed_threshold_key, tau): min(slots), and with a guess the
    rank-th LARGEST slot (set_guess ranks by counting; an empty slot is -inf)"""
    lowest = slots.min(axis=1)
    if rank is None:
        return lowest
    return np.maximum(lowest, -np.sort(-slots, axis=1)[:, rank - 1])


# ---- brackets ---------------------------------------------------------------------------------------------------------------------------
def counts(parts, qs, tau, screen, mid, D, sgn, e=0.0):
    """The model's survivor counts of one pass, summed over its queries: every test at tau - sgn e, loosened (sgn = +1) or tightened
    (sgn = -1) by its slack; sgn = 0: the tests themselves at tau.  mid: None | the reader of the mid copy (screens_ref.mid_reader)."""
    sl = sr.slacks(D, mid or "drain_survivors")
    t = np.maximum(np.asarray(tau, dtype=np.float64) - sgn * e, -1e30)  # (-inf, a group without a row: everything passes; no inf - inf)
    tot = {"coarse": 0, "candidates": 0}
    if mid:
        tot["mid"] = 0
    for rows in parts:
        fine = keep_fine(rows, qs, t, sgn * sl["fine"])
        if screen == "wave":
            coarse = np.ones_like(fine)
        elif screen == "int8":
            coarse = keep_int8(rows, qs, t, sgn * sl["int8"])
        else:
            coarse = keep_bf16(rows, qs, t, sgn * sl[screen], f32_rows=screen == "f32")
        left = coarse
        if mid:
            left = coarse & keep_mid(rows, qs, t, sgn * sl["mid"])
            tot["mid"] += int(left.sum())
        tot["coarse"] += int(coarse.sum())
        tot["candidates"] += int((left & fine).sum())
    if screen == "wave":
        tot.pop("coarse")  # (the wave kernel counts candidates only)
    return tot


def bracket(parts, qs, tau, screen, mid, D):
    """{name: (lo, hi)} at the start threshold tau [B] of a pass"""
    e = eps32(D) * qs.unit
    lo, hi = counts(parts, qs, tau, screen, mid, D, -1.0, e), counts(parts, qs, tau, screen, mid, D, 1.0, e)
    return {name: (lo[name], hi[name]) for name in lo}


# ---- the shapes of tests/test_seed_gpu.py -----------------------------------------------------------------------------------------------
# screen: "int8" (the int8 copy, AUTO's kernel), "f32" (no copy, set_kernel("mfma"): what a search over more than 1 024 features
# streams, fill_segment_table), "bf16" (the bf16 copy), "wave" (no copy, up to four queries).  flags: the tuning word.
Shape = namedtuple("Shape", "form D B k flags screen mid rows")
N8, ONE_PART = sr.TUNE_NO_SIX, with_parts(1)
PIN = FLAG_NO_GUESS | ONE_PART  # a pinned pass: no guess; one seed part = 8 seed blocks, at 94 blocks every 8th
VALU16 = FLAG_SEED16 | FLAG_VALU_SEED


def _pinned():
    out = [Shape("mfma", 128, 8, 10, N8 | PIN, "int8", "off", 3007), Shape("mfma", 128, 64, 10, N8 | PIN, "int8", "on", 3007),
           Shape("mfma", 1152, 32, 81, PIN, "f32", "off", 3007), Shape("mfma", 1216, 32, 17, PIN, "f32", "off", 3007),
           Shape("mfma", 1152, 32, 82, PIN, "f32", "off", 3007), Shape("mfma", 1216, 32, 18, PIN, "f32", "off", 3007),
           Shape("mfma", 1152, 32, 92, PIN, "f32", "off", 3007), Shape("valu8", 1152, 32, 93, PIN, "f32", "off", 3007),
           Shape("mfma", 1216, 32, 28, PIN, "f32", "off", 3007), Shape("valu8", 1216, 32, 29, PIN, "f32", "off", 3007),
           Shape("valu8", 1280, 32, 10, PIN, "f32", "off", 3007),  # the first width the MFMA seed never takes
           Shape("valu8", 1536, 5, 64, PIN, "f32", "off", 3007), Shape("valu8", 1536, 32, 10, PIN, "f32", "off", 3007),
           Shape("valu8", 128, 8, 10, N8 | PIN | FLAG_VALU_SEED, "int8", "off", 3007),
           Shape("valu1", 2048, 7, 32, PIN, "f32", "off", 3007), Shape("valu1", 2496, 32, 10, PIN, "f32", "off", 3007),
           Shape("valu1", 128, 1, 128, PIN | FLAG_VALU_SEED, "wave", "off", 3007), Shape("valu1", 128, 2, 110, PIN | FLAG_VALU_SEED, "wave", "off", 3007)]
    out += [Shape("valu16", D, B, 10, N8 | PIN | VALU16, "int8", "off", 3007) for D in (384, 896) for B in (33, 64)]
    out.append(Shape("mfma", 128, 64, 10, N8 | FLAG_NO_GUESS, "int8", "off", 40_000))  # the default 64 parts: 512 of 1 250 blocks, every 2nd
    return out


PINNED = _pinned()
GUESS = [Shape("mfma", D, B, k, (N8 if screen == "int8" else 0) | FLAG_NO_LEARNED | ONE_PART, screen, "off", 20_000)
         for D, screen in ((128, "int8"), (640, "bf16")) for B in (5, 64) for k in (2, 10, 128)]
METRICS = ("cosine", "dot")


def padded(D):
    return (D + 63) // 64 * 64


def form_of(shape):
    return seed_form(shape.B, padded(shape.D), shape.k, shape.flags)


def scan_of(shape):
    return scan_form(shape.B, shape.D, shape.flags, shape.screen)


def mid_of(shape):
    return sr.mid_reader(scan_of(shape)) if shape.mid == "on" else None


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _near(rng, centre, t):
    """rows at cosine t [n] with the unit vector `centre`: t centre + sqrt(1 - t^2) u, u a unit vector orthogonal to it"""
    u = rng.standard_normal((len(t), len(centre)))
    u = _unit(u - (u @ centre)[:, None] * centre[None, :])
    return t[:, None] * centre[None, :] + np.sqrt(1.0 - t ** 2)[:, None] * u


RADIUS = 1.5  # dot: the norm of every planted and ladder row, and the largest in the corpus


def _background(rng, n, D, metric):
    """Gaussian rows: cosines of some 1 / sqrt(D) with anything; norms 0.5 .. 2 (cosine), 0.5 .. 1 of RADIUS (dot)"""
    g = rng.standard_normal((n, D))
    if metric == "dot":
        return _unit(g) * RADIUS * rng.uniform(0.5, 1.0, (n, 1))
    return g * rng.uniform(0.5, 2.0, (n, 1)) / np.sqrt(D)


class Pinned:
    """The planted corpus of a pinned shape.  The B queries fall in G clusters (query b: cluster b % G), each a near-copy of its
    cluster's centre; cluster g has k planted rows at cosines above 0.80 + 0.012 g with the centre, one in each of the k seed
    groups, in seed blocks spread over the sample; below the lowest of them a ladder of near-copies of the centre (`spans`: how
    far below), anywhere in the corpus, on a Gaussian background with an all-zero row and a row with an inf in seed blocks.  Rows other than
    the planted ones that come within GAP eps32 unit of a query's k-th best are redrawn as background: afterwards the k best rows
    of every query are its cluster's planted rows, min(slots) is the k-th best score, and no other row has an f32 score above it
    (two f32 chains of D features differ from the float64 scores by eps32 unit each at most), so no offer of the scan raises tau."""

    GAP = 8.0
    _all = {}

    @classmethod
    def get(cls, shape, metric):
        key = (shape.D, shape.B, shape.k, shape.flags & 0xFF0000, shape.screen, shape.mid, shape.rows, metric)
        if key not in cls._all:
            cls._all[key] = cls(shape, metric)
        return cls._all[key]

    def __init__(self, shape, metric):
        D, B, k, n = shape.D, shape.B, shape.k, shape.rows
        self.shape, self.metric, self.D, self.B, self.k = shape, metric, D, B, k
        self.plan = seed_plan(n, shape.flags)
        sample, srow = seed_sample(n, self.plan)
        rng = np.random.default_rng(9100 + D + 7 * B + 131 * k + (1 if metric == "dot" else 0))
        per_group = [sample[sample % k == j] for j in range(k)]
        G = self.G = min(B, 8, min(len(a) for a in per_group), (len(sample) - 2) // k)  # (two seed rows stay free: the edge rows)
        assert G >= 1
        row_of = dict(zip(sample.tolist(), srow.tolist()))
        # cluster g, group j: the sample position of group j at the fraction (g + 0.5) / G + 0.618034 j (mod 1) of the sample: the
        # clusters apart, the groups hopping by the golden ratio, so that the planted rows lie over ALL the seed blocks, the
        # first and the last included (a skipped block shows)
        self.planted = np.array([[row_of[int(per_group[j][int(((g + 0.5) / G + 0.618034 * j) % 1.0 * len(per_group[j]))])] for j in range(k)]
                                 for g in range(G)])
        assert len(np.unique(self.planted)) == G * k
        wide = shape.screen != "int8"
        e = eps32(D)
        ladder = (60 if wide else 2000 // G) if n < 10_000 else 1500
        if wide:
            # the bf16 screen's band (margin = eps16 + eps32 = 0.0039101 + 3 eps32 of a unit) is no wider than a few of its own
            # slacks at these widths: half the ladder lies in the part of the band that is kept at either end of the bracket,
            # half clearly outside it (zone: e and the slack at tau ~ 0.8, and what a query's own direction adds to a cosine)
            band, zone = 0.0039101 + 3 * e, 3 * e + 0.03 / np.sqrt(D)
            spans = [(max(0.002, 9 * e), band - zone), (band + zone, band + zone + 0.005)]
        else:
            # the int8 test's band is some 0.02 of a cosine at every width; its slack grows with eps32, and above 512 features a
            # ladder across the band's edge leaves more than 2 % of the count open: there the ladder stays clear of the edge
            spans = [(0.003, 0.08)] if D <= 512 else [(0.003, 0.010), (0.04, 0.08)]
        spans = [(a, b) for a, b in spans if a < b]
        level = 0.80 + 0.012 * np.arange(G)
        centres = _unit(rng.standard_normal((G, D)))
        self.cluster = np.arange(B) % G
        q = centres[self.cluster] + 0.01 * _unit(rng.standard_normal((B, D)))
        self.queries = (q * rng.uniform(0.5, 2.0, (B, 1))).astype(np.float32)
        x = _background(rng, n, D, metric)
        free = np.setdiff1d(np.arange(n), self.planted.reshape(-1))
        seed_free = np.setdiff1d(srow, self.planted.reshape(-1))
        self.zero_row, self.inf_row = int(seed_free[0]), int(seed_free[-1])
        free = np.setdiff1d(free, [self.zero_row, self.inf_row])
        ladder = ladder // len(spans) * len(spans)
        spots = rng.permutation(free)[: G * ladder].reshape(G, ladder)
        scale = RADIUS if metric == "dot" else 1.0
        for g in range(G):
            top = level[g] + (0.985 - level[-1]) * (np.arange(k) + 1.0) / (k + 1.0)
            x[self.planted[g]] = _near(rng, centres[g], top) * (scale if metric == "dot" else rng.uniform(0.5, 2.0, (k, 1)))
            t = top[0] - np.concatenate([rng.uniform(a, b, ladder // len(spans)) for a, b in spans])
            x[spots[g]] = _near(rng, centres[g], t) * (scale if metric == "dot" else rng.uniform(0.5, 2.0, (ladder, 1)))
        x = x.astype(np.float32)
        x[self.zero_row] = 0.0
        x[self.inf_row, 1] = np.inf
        mine = np.zeros((n, B), bool)  # the planted rows of each query
        for b in range(B):
            mine[self.planted[self.cluster[b]], b] = True
        for _ in range(6):  # redraw what comes too close to a k-th best
            rows = Rows(x, metric)
            qs = Queries(self.queries, rows)
            s = np.where(np.isfinite(scores64(rows, qs)[:n]) & (rows.scale[:n] != 0)[:, None], scores64(rows, qs)[:n], -np.inf)
            kth = np.where(mine, s, np.inf).min(axis=0)
            close = ((s >= kth[None, :] - self.GAP * e * qs.unit[None, :]) & ~mine).any(axis=1)
            if not close.any():
                break
            x[close] = _background(rng, int(close.sum()), D, metric).astype(np.float32)
        assert not close.any()
        self.corpus, self.rows, self.qs, self.kth = x, rows, qs, kth
        self.kth_row = np.where(mine, s, np.inf).argmin(axis=0)
        self.best_row = np.where(mine, s, -np.inf).argmax(axis=0)
        self.slots = seed_slots(rows, qs, k, self.plan)
        self.tau = tau_start(self.slots, None)
        self._bracket = None

    def bracket(self):
        if self._bracket is None:
            self._bracket = bracket([self.rows], self.qs, self.tau, self.shape.screen, mid_of(self.shape), self.D)
        return self._bracket

    def faulty(self, fault):
        """the model's counts, every test tightened, at the start threshold of a seed with one fault: "lost" — the k-th planted
        row of every query goes unseen (its group is lost: a skipped block, a slot never filled); "shared" — the best planted row
        is ranked in the k-th's group, two rows in one slot and none in its own"""
        if fault == "lost":
            slots = seed_slots(self.rows, self.qs, self.k, self.plan, drop=self.kth_row)
        else:
            sample, srow = seed_sample(self.rows.n, self.plan)
            group = dict(zip(srow.tolist(), (sample % self.k).tolist()))
            slots = seed_slots(self.rows, self.qs, self.k, self.plan, move=(self.best_row, [group[int(r)] for r in self.kth_row]))
        tau = tau_start(slots, None)
        return tau, counts([self.rows], self.qs, tau, self.shape.screen, mid_of(self.shape), self.D, -1.0, eps32(self.D) * self.qs.unit)


class Guess:
    """The planted corpus of the guess shapes at (D, k, metric): 20 000 Gaussian rows and 64 Gaussian queries, for each query k
    near-copies at cosines 0.55 .. 0.9 in rows OUTSIDE the seed blocks.  The seed rows are background to every query, so the
    rank-th largest slot is a few standard deviations of a background score and the planted rows stand far above it: the check of
    the guess (rescore_select_kernel: k rows at guess + margin32) holds, and the pass needs no repeat."""

    _all = {}

    @classmethod
    def get(cls, shape, metric):
        key = (shape.D, shape.k, shape.flags & 0xFF0000, shape.rows, metric)
        if key not in cls._all:
            cls._all[key] = cls(shape, metric)
        return cls._all[key]

    def __init__(self, shape, metric):
        D, k, n, B = shape.D, shape.k, shape.rows, 64
        self.metric, self.D, self.k = metric, D, k
        self.plan = seed_plan(n, shape.flags)
        sample, srow = seed_sample(n, self.plan)
        self.rank = guess_rank(k, n, min(n, self.plan[0] * BLOCK_ROWS))
        rng = np.random.default_rng(9700 + D + 131 * k + (1 if metric == "dot" else 0))
        x = _background(rng, n, D, metric)
        q = rng.standard_normal((B, D))
        blocks = np.arange((n + 31) // 32)
        in_seed = np.isin(blocks, (np.arange(self.plan[0]) << self.plan[1]))
        free = np.flatnonzero(~np.repeat(in_seed, 32)[:n])
        self.planted = rng.permutation(free)[: B * k].reshape(B, k)
        for b in range(B):
            rows = _near(rng, _unit(q[b]), np.linspace(0.9, 0.55, k))
            x[self.planted[b]] = rows * (RADIUS if metric == "dot" else rng.uniform(0.5, 2.0, (k, 1)))
        self.corpus = x.astype(np.float32)
        self.queries = (q * rng.uniform(0.5, 2.0, (B, 1))).astype(np.float32)
        self.rows = Rows(self.corpus, metric)
        self._runs = {}

    def run(self, shape):
        """(qs, slots, tau at the guess, tau at min(slots)) of the pass of the first shape.B queries"""
        if shape.B not in self._runs:
            qs = Queries(self.queries[: shape.B], self.rows)
            slots = seed_slots(self.rows, qs, self.k, self.plan)
            self._runs[shape.B] = (qs, slots, tau_start(slots, self.rank), tau_start(slots, None))
        return self._runs[shape.B]

    def high(self, shape):
        """{name: hi}: the high end of the bracket at the model's start threshold"""
        qs, _, tau, _ = self.run(shape)
        return counts([self.rows], qs, tau, shape.screen, None, self.D, 1.0, eps32(self.D) * qs.unit)

    def low_without(self, shape):
        """{name: lo}: the low end at min(slots), what a pass whose guess was not applied starts from"""
        qs, _, _, lowest = self.run(shape)
        return counts([self.rows], qs, lowest, shape.screen, None, self.D, -1.0, eps32(self.D) * qs.unit)
