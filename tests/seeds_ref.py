"""What the seed-item tests share (test_seeds_cpu.py, test_seeds_gpu.py): the reference of pcv_searcher_seeds and the comparison
with it.  A plain module, like neighbors_ref.py, whose corpus helpers the tests use beside it.

The reference of every check is orc_canonical_score(row_r, row_s, D, 0) of every participating row r with every seed s, cached per
seed; the integer weights are numpy's rint on f64, the prefix sums and the draw are Python ints.  `brute_force` follows the
definition line by line, without the cache and without numpy arithmetic."""
import bisect
import ctypes as C
import itertools

import numpy as np

from duplicates_ref import bits
from neighbors_ref import takes_part

_FP = C.POINTER(C.c_float)
_M = (1 << 64) - 1
METHODS = ("kmeans++", "farthest")


def seed_draw(seed, step, total):
    """floor(z * total / 2^64), z the splitmix64 finaliser of seed + (step + 1) * 0x9E3779B97F4A7C15 (mod 2^64)"""
    z = (seed + (step + 1) * 0x9E3779B97F4A7C15) & _M
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M
    z ^= z >> 31
    return (z * total) >> 64


def weights(cover):
    """w = (int64) rint(max(0, 1 - cover) * 2^32), ties to even, from an f64 array"""
    return np.rint(np.maximum(0.0, 1.0 - np.asarray(cover, dtype=np.float64)) * 2.0 ** 32).astype(np.int64)


class Reference:
    """The reference over one set of rows (in global position order); the cosines with a seed are computed once."""

    def __init__(self, oracle, rows, ids, part=None, positions=None):
        self.oracle = oracle
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.n, self.dim = self.rows.shape
        self.ids = np.asarray(ids, dtype=np.int64)
        self.positions = np.arange(self.n, dtype=np.int64) if positions is None else np.asarray(positions, dtype=np.int64)
        self.live = np.nonzero(takes_part(self.rows, part))[0]
        self._ptr = [C.cast(self.rows.ctypes.data + int(r) * self.dim * 4, _FP) for r in range(self.n)]
        self._col = {}

    def column(self, s):
        """c(r, s) for every participating r, f64"""
        if s not in self._col:
            f = self.oracle.lib.orc_canonical_score
            self._col[s] = np.array([f(self._ptr[int(r)], self._ptr[s], self.dim, 0) for r in self.live], dtype=np.float64)
        return self._col[s]

    def picks(self, k, method, seed=0, first_id=None):
        """-> (indices into the participating rows, totals, f64 cover of each pick (NaN at step 0)); ValueError: first_id is nobody's"""
        assert method in METHODS
        live = self.live
        chosen, totals, covers = [], [], []
        cover = None
        for j in range(k):
            w = [1] * live.size if j == 0 else weights(cover).tolist()
            T = sum(w)
            if T == 0:
                break
            if j == 0 and first_id is not None:
                carry = np.nonzero(self.ids[live] == first_id)[0]
                if carry.size == 0:
                    raise ValueError("first_id")
                i = int(carry[0])
            elif method == "farthest":
                i = w.index(max(w))
            else:
                i = bisect.bisect_right(list(itertools.accumulate(w)), seed_draw(seed, j, T))
            chosen.append(i)
            totals.append(T)
            covers.append(np.nan if j == 0 else cover[i])
            c = self.column(int(live[i]))
            cover = c.copy() if cover is None else np.maximum(cover, c)
        return chosen, totals, covers

    def seeds(self, k, method, seed=0, first_id=None):
        """-> (ids, positions, totals int64, cover f32), cut to the count, as Searcher.seeds returns them"""
        chosen, totals, covers = self.picks(k, method, seed, first_id)
        r = self.live[chosen] if chosen else np.zeros(0, dtype=np.int64)
        return self.ids[r], self.positions[r], np.array(totals, dtype=np.int64), np.array(covers, dtype=np.float64).astype(np.float32)


def reference(oracle, rows, ids, k, method, seed=0, first_id=None, part=None, positions=None):
    return Reference(oracle, rows, ids, part, positions).seeds(k, method, seed, first_id)


def check(got, want):
    g_ids, g_pos, g_tot, g_cov = got
    w_ids, w_pos, w_tot, w_cov = want
    print("seeds %d/%d" % (len(g_ids), len(w_ids)))
    assert g_ids.dtype == np.int64 and g_pos.dtype == np.int64 and g_tot.dtype == np.int64 and g_cov.dtype == np.float32
    np.testing.assert_array_equal(g_ids, w_ids)  # (the count with them)
    np.testing.assert_array_equal(g_pos, w_pos)
    np.testing.assert_array_equal(g_tot, w_tot)
    assert len(g_cov) == len(w_cov)
    if len(w_cov):
        assert np.isnan(g_cov[0]) and np.isnan(w_cov[0])
        np.testing.assert_array_equal(bits(g_cov[1:]), bits(w_cov[1:]))


def brute_force(oracle, rows, ids, k, method, seed=0, first_id=None, part=None):
    """the definition itself, every weight of every step through the oracle: for small inputs, to check `Reference`"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    live = [int(r) for r in np.nonzero(takes_part(rows, part))[0]]
    seeds, out = [], []
    for j in range(k):
        cover = [None if j == 0 else max(oracle.canonical_score(rows[r], rows[s]) for s in seeds) for r in live]
        w = [1 if j == 0 else int(round(max(0.0, 1.0 - c) * 2.0 ** 32)) for c in cover]  # (round: ties to even)
        T = sum(w)
        if T == 0:
            break
        if j == 0 and first_id is not None:
            carry = [i for i, r in enumerate(live) if ids[r] == first_id]
            if not carry:
                raise ValueError("first_id")
            i = carry[0]
        elif method == "farthest":
            i = max(range(len(live)), key=lambda x: (w[x], -x))
        else:
            t = seed_draw(seed, j, T)
            run, i = 0, None
            for x, wx in enumerate(w):
                run += wx
                if run > t:
                    i = x
                    break
        seeds.append(live[i])
        out.append((int(ids[live[i]]), live[i], T, np.float32(np.nan if j == 0 else cover[i])))
    return (np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out], dtype=np.int64),
            np.array([o[2] for o in out], dtype=np.int64), np.array([o[3] for o in out], dtype=np.float32))
