"""Host-side mirror of perceive-core's search module (crates/perceive-core/search.rs) over the
C ABI.  Same names and argument meaning as the reference; the SQLite `Database` argument of
`Searcher::build` / `rebuild_source` is replaced by the row stream its SQL produces
(search.rs:87-113: `(items.id, source_id, embedding blob)`), because storage is out of scope.
"""
import ctypes as C
import weakref
from dataclasses import dataclass

import numpy as np

from . import _ffi
from .context import Context

PCV_MAX_DISTINCT_POOL = 4096  # include/perceive_hip.h
PCV_MAX_DIVERSE_POOL = 4096  # include/perceive_hip.h
PCV_MAX_GROUPED_POOL = 4096  # include/perceive_hip.h
PCV_NO_GROUP = -1  # include/perceive_hip.h: "no group" in set_groups / groups_of / search_grouped
PCV_MAX_WHERE_POOL = 4096  # include/perceive_hip.h
PCV_NO_VALUE = -(1 << 63)  # include/perceive_hip.h: "no value" in set_values / values_of / search_where
WHERE_UNSET_PASSES, WHERE_OUTSIDE = 1, 2  # include/perceive_hip.h: PCV_WHERE_*, the flags of a predicate
PCV_MAX_BOOST_KNOTS = 16  # include/perceive_hip.h: most knots of a boost (search_boosted)
PCV_MAX_BOOST_POOL = 4096  # include/perceive_hip.h
PCV_MAX_COMPOUND_PARTS = 8  # include/perceive_hip.h: most wanted, and most avoided, vectors of a compound (search_compound)
PCV_MAX_COMPOUND_POOL = 4096  # include/perceive_hip.h
COMPOUND_MODES = {"all": 0, "any": 1}  # include/perceive_hip.h: PCV_COMPOUND_ALL, PCV_COMPOUND_ANY
PCV_MAX_DUPLICATE_PAIRS = 1 << 24  # include/perceive_hip.h
PCV_MAX_NEIGHBORS = 64  # include/perceive_hip.h
GROUPS_SKIP_OWN, GROUPS_ONE_PER_GROUP = 1, 2  # include/perceive_hip.h: PCV_GROUPS_*, the flags of the grouped pair calls
PCV_MAX_SEEDS = 4096  # include/perceive_hip.h
PCV_DENSITY_NONE, PCV_DENSITY_NOISE, PCV_DENSITY_BORDER, PCV_DENSITY_CORE = -1, 0, 1, 2  # include/perceive_hip.h: out_kind
PCV_MAX_AXES = 64  # include/perceive_hip.h
_SEED_METHODS = {"farthest": 0, "kmeans++": 1}  # PCV_SEED_FARTHEST, PCV_SEED_KMEANSPP

_METRICS = {"cosine": _ffi.METRIC_COSINE, "dot": _ffi.METRIC_DOT}
_KERNELS = {"auto": _ffi.KERNEL_AUTO, "wave": _ffi.KERNEL_WAVE, "mfma": _ffi.KERNEL_MFMA}
STAGING_SOURCE = -(1 << 63)  # PCV_STAGING_SOURCE


@dataclass(frozen=True)
class SearchItem:
    """search.rs:18-22"""

    id: int
    score: float


def serialize_embedding(embedding):
    """search.rs:288-294 — little-endian f32 bytes, no header."""
    v = np.ascontiguousarray(embedding, dtype=np.float32)
    out = np.empty(v.size * 4, dtype=np.uint8)
    _ffi.check(_ffi.lib().pcv_serialize_embedding(_ffi.f32p(v), v.size, _ffi.u8p(out), out.size))
    return out.tobytes()


def deserialize_embedding(value):
    """search.rs:281-286"""
    b = np.frombuffer(bytes(value), dtype=np.uint8)
    out = np.empty(len(b) // 4, dtype=np.float32)
    n = C.c_size_t()
    _ffi.check(_ffi.lib().pcv_deserialize_embedding(_ffi.u8p(b), b.size, _ffi.f32p(out), out.size, C.byref(n)))
    return out[: n.value]


def _source_filter(sources):
    """(pointer, count, keep-alive) of a source filter for the C ABI: None -> NULL (all sources); a list ->
    exactly those, an empty list matching nothing (search.rs:166).  The pointer of an empty list is still
    non-NULL."""
    if sources is None:
        return None, 0, None
    sa = np.ascontiguousarray(list(sources), dtype=np.int64)
    n = int(sa.size)
    if n == 0:
        sa = np.zeros(1, dtype=np.int64)
    return _ffi.i64p(sa), n, sa


def recency_boost(now, half_life, weight, knots=PCV_MAX_BOOST_KNOTS):
    """Knots for search_boosted that sample weight * 2 ** -((now - v) / half_life): -> (knot_values, knot_boosts), values
    ascending.  The last knot is at `now` (boost `weight`: newer items get no more); going back, knot i lies
    round(half_life * (2 ** (i / 3) - 1)) before `now` (one more where that would repeat an age), so the gaps grow geometrically —
    fine where the curve bends, 31 half-lives back with 16 knots — and items older than the first knot keep its boost.  A plain
    function of its arguments: `now` and `half_life` are integers in the unit of the stored values."""
    now, half_life, knots = int(now), int(half_life), int(knots)
    if half_life < 1 or not 1 <= knots <= PCV_MAX_BOOST_KNOTS:
        raise ValueError("half_life must be >= 1 and knots in [1, PCV_MAX_BOOST_KNOTS]")
    ages = []
    for i in range(knots):
        age = int(round(half_life * (2.0 ** (i / 3.0) - 1.0)))
        ages.append(age if not ages else max(age, ages[-1] + 1))
    if now - ages[-1] <= PCV_NO_VALUE:
        raise ValueError("the oldest knot falls below the smallest value")
    values = [now - a for a in reversed(ages)]
    boosts = [float(weight) * 2.0 ** -(a / half_life) for a in reversed(ages)]
    return values, boosts


class Searcher:
    """search.rs:29-35.  One exact, GPU-resident index per process; sources are kept apart so
    `search_vector(sources=...)` filters like search.rs:166 and `rebuild_source` replaces one.

    metric="dot"    -> the reference Searcher's convention: score = max(0, 1 - dot/len)
                       (search.rs:269-278), results ascending by score (search.rs:179).
    metric="cosine" -> lib.rs:67-77 cosine, results best (largest) first.
    """

    def __init__(self, ctx: Context, dim: int, metric: str = "cosine"):
        self.ctx = ctx
        self.dim = int(dim)
        self.metric = metric
        self._h = C.c_void_p()
        _ffi.check(_ffi.lib().pcv_searcher_create(ctx.handle, self.dim, _METRICS[metric], C.byref(self._h)))
        ctx._register(self)
        # search.rs:31-34: ids hidden after the index was built.  Kept, and (like the reference's
        # search_vector) not consulted when searching.
        self.hidden = set()

    # ---- construction -------------------------------------------------------------------------
    @classmethod
    def build(cls, ctx, rows, dim, metric="cosine"):
        """Searcher::build (search.rs:38-56).  `rows` yields (item_id, source_id, embedding) with the
        embedding as a blob (bytes) or a float array — what the query at search.rs:87-113 returns."""
        s = cls(ctx, dim, metric)
        s._insert(rows)
        s.finalize()
        return s

    def rebuild_source(self, rows, source_id):
        """Searcher::rebuild_source (search.rs:58-79): rows of other sources are ignored
        (search.rs:106-109); an empty replacement leaves the source absent."""
        # search.rs:57-79 builds the new index first and swaps it in only once it exists: the replacement is staged
        # under PCV_STAGING_SOURCE, so that a bad row leaves the old rows of the source in place
        lib, staging = _ffi.lib(), STAGING_SOURCE
        _ffi.check(lib.pcv_searcher_clear_source(self._handle, staging))
        try:
            self._insert((r for r in rows if int(r[1]) == int(source_id)), into=staging)
            self.finalize()
        except Exception:
            lib.pcv_searcher_clear_source(self._handle, staging)
            lib.pcv_searcher_finalize(self._handle)
            raise
        _ffi.check(lib.pcv_searcher_replace_source(self._handle, staging, int(source_id)))
        self.finalize()

    def _insert(self, rows, into=None):
        by_source = {}
        for item_id, source_id, emb in rows:
            v = deserialize_embedding(emb) if isinstance(emb, (bytes, bytearray, memoryview)) else np.asarray(
                emb, dtype=np.float32
            )
            if v.shape != (self.dim,):
                raise ValueError(f"embedding of item {item_id} has shape {v.shape}, index is {self.dim}-d")
            ids, vecs = by_source.setdefault(int(source_id) if into is None else into, ([], []))
            ids.append(int(item_id))
            vecs.append(v)
        for source_id, (ids, vecs) in by_source.items():
            self.add_rows(source_id, np.stack(vecs), np.asarray(ids, dtype=np.int64))

    def add_rows(self, source_id, rows, ids=None):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}]")
        idp = None
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.int64)
            if ids.shape != (rows.shape[0],):
                raise ValueError("ids must be [n]")
            idp = _ffi.i64p(ids)
        _ffi.check(_ffi.lib().pcv_searcher_add_rows(self._handle, int(source_id), idp, _ffi.f32p(rows), rows.shape[0]))

    def add_blobs(self, source_id, blobs: bytes, n, ids=None):
        b = np.frombuffer(blobs, dtype=np.uint8)
        if b.size != n * self.dim * 4:
            raise ValueError("blob bytes do not match n*dim*4")
        idp = None
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.int64)
            idp = _ffi.i64p(ids)
        _ffi.check(_ffi.lib().pcv_searcher_add_blobs(self._handle, int(source_id), idp, _ffi.u8p(b), int(n)))

    def reserve(self, source_id, n_rows):
        """Announce that `n_rows` more rows are about to be added to `source_id` (one device segment for them)."""
        _ffi.check(_ffi.lib().pcv_searcher_reserve(self._handle, int(source_id), int(n_rows)))

    def add_synthetic(self, source_id, n, seed, first_row=0, normalize=False, n_clusters=0, noise=0.0, amplitude=None):
        """Rows generated on the device.  n_clusters > 0: clustered rows (centroid/sqrt(dim) + noise * row);
        amplitude=(lo, hi): un-normalised rows a(row) * row with a uniform in [lo, hi) (norms spread: dot-metric corpora)."""
        if amplitude is not None:
            _ffi.check(_ffi.lib().pcv_searcher_add_synthetic_scaled(self._handle, int(source_id), int(n), int(seed), int(first_row),
                                                                  float(amplitude[0]), float(amplitude[1])))
            return
        _ffi.check(
            _ffi.lib().pcv_searcher_add_synthetic_clustered(
                self._handle, int(source_id), int(n), int(seed), int(first_row), 1 if normalize else 0,
                int(n_clusters), float(noise)
            )
        )

    def finalize(self):
        _ffi.check(_ffi.lib().pcv_searcher_finalize(self._handle))

    # ---- queries ------------------------------------------------------------------------------
    def search_vector(self, sources, num_results, vector):
        """Searcher::search_vector (search.rs:157-182)."""
        ids, scores, counts = self.search_vectors(sources, num_results, np.asarray(vector, dtype=np.float32)[None, :])
        return [SearchItem(int(ids[0, j]), float(scores[0, j])) for j in range(int(counts[0]))]

    def search_vectors(self, sources, num_results, vectors):
        """Batched search_vector: vectors [B, dim] -> (ids [B,k] int64, scores [B,k] f32, counts [B])."""
        q = np.ascontiguousarray(vectors, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"vectors must be [B, {self.dim}]")
        B, k = q.shape[0], int(num_results)
        ids = np.full((B, k), -1, dtype=np.int64)
        scores = np.full((B, k), np.nan, dtype=np.float32)
        counts = np.zeros(B, dtype=np.int32)
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_search(
                self._handle, _ffi.f32p(q), B, src, nsrc, k, _ffi.i64p(ids), _ffi.f32p(scores),
                _ffi.i32p(counts),
            )
        )
        return ids, scores, counts

    def search(self, model, sources, num_results, query):
        """Searcher::search (search.rs:184-193)."""
        return self.search_vector(sources, num_results, encode_query(model, query))

    def search_device(self, sources, num_results, vectors, d_out, async_=False):
        """Per-shard exact top-k left on the device: d_out = device pointer to [B][k] pcv_hit."""
        q = np.ascontiguousarray(vectors, dtype=np.float32)
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_device(
                self._handle, _ffi.f32p(q), q.shape[0], src, nsrc, int(num_results), C.c_void_p(d_out),
                1 if async_ else 0,
            )
        )

    def search_device_begin(self, sources, num_results, vectors, d_out):
        """Queue the per-shard pass without waiting (pcv_searcher_search_device_begin): d_out receives
        B*k hits + one overflow record.  Raises PcvError(status 3) if it needs more than one pass."""
        q = np.ascontiguousarray(vectors, dtype=np.float32)
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_device_begin(
                self._handle, _ffi.f32p(q), q.shape[0], src, nsrc, int(num_results), C.c_void_p(d_out)
            )
        )

    def search_device_begin_dq(self, sources, num_results, d_queries, n_queries, d_out):
        """The same with the queries in device memory (pcv_searcher_search_device_begin_dq): `d_queries` is the address of
        [n_queries][dim] f32 on this searcher's device, e.g. what Model.encode_tokens_device left there."""
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_device_begin_dq(
                self._handle, C.c_void_p(d_queries), int(n_queries), src, nsrc, int(num_results), C.c_void_p(d_out)
            )
        )

    def search_device_end(self):
        """Wait for the queued pass and book its statistics; True if the pass has to be repeated (a candidate list
        overflowed, or a speculative start threshold did not hold)."""
        over = C.c_int()
        _ffi.check(_ffi.lib().pcv_searcher_search_device_end(self._handle, C.byref(over)))
        return bool(over.value)

    def repeat_without_guess(self):
        """A sharded step is repeated because some rank's pass was incomplete: this rank's repeat runs without a
        speculative start threshold too (pcv_searcher_repeat_without_guess)."""
        _ffi.check(_ffi.lib().pcv_searcher_repeat_without_guess(self._handle))

    def search_sharded(self, comm, sources, num_results, vectors):
        """Collective exact top-k over every rank's shard (pcv_searcher_search_sharded): local pass,
        RCCL all-gather of the hit lists, merge.  Returns (ids[B,k], scores[B,k], counts[B])."""
        q = np.ascontiguousarray(vectors, dtype=np.float32)
        B, k = q.shape[0], int(num_results)
        src, nsrc, _keep = _source_filter(sources)
        ids = np.full((B, k), -1, dtype=np.int64)
        scores = np.full((B, k), np.nan, dtype=np.float32)
        counts = np.zeros(B, dtype=np.int32)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_sharded(
                self._handle, comm._handle, _ffi.f32p(q), B, src, nsrc, k, _ffi.i64p(ids), _ffi.f32p(scores),
                _ffi.i32p(counts),
            )
        )
        return ids, scores, counts

    def search_sharded_dq(self, comm, sources, num_results, d_queries, n_queries):
        """search_sharded with the queries in device memory, the same on every rank (pcv_searcher_search_sharded_dq)."""
        B, k = int(n_queries), int(num_results)
        src, nsrc, _keep = _source_filter(sources)
        ids = np.full((B, k), -1, dtype=np.int64)
        scores = np.full((B, k), np.nan, dtype=np.float32)
        counts = np.zeros(B, dtype=np.int32)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_sharded_dq(
                self._handle, comm._handle, C.c_void_p(d_queries), B, src, nsrc, k, _ffi.i64p(ids), _ffi.f32p(scores),
                _ffi.i32p(counts),
            )
        )
        return ids, scores, counts

    # ---- search by example (pcv_searcher_like_queries / _search_like) ------------------------------
    # `perceive search --like <id>` (cmd/search.rs:64-86): the query is the stored embedding of an item, or a weighted sum of
    # several, built on the device from the rows this searcher holds.  A view looks the examples up in its parent.
    @staticmethod
    def _like_args(groups, weights):
        """groups: a list of id lists, one per query; weights: None (all 1), or the same shape, or flat over all examples.
        -> (ids int64 [n], weights f32 [n] or None, offsets int64 [len(groups) + 1])"""
        groups = [np.asarray(g, dtype=np.int64).reshape(-1) for g in groups]
        offsets = np.zeros(len(groups) + 1, dtype=np.int64)
        if groups:
            np.cumsum([g.size for g in groups], out=offsets[1:])
        ids = np.ascontiguousarray(np.concatenate(groups) if groups else np.zeros(0, dtype=np.int64), dtype=np.int64)
        w = None
        if weights is not None:
            if len(weights) == len(groups) and all(np.ndim(x) == 1 for x in weights):
                weights = np.concatenate([np.asarray(x, dtype=np.float32) for x in weights]) if groups else []
            w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
            if w.size != ids.size:
                raise ValueError(f"{w.size} weights for {ids.size} examples")
        return ids, w, offsets

    def like_queries(self, groups, weights=None, d_out=None):
        """Query vectors made from stored items: query q is sum_i weights[q][i] * (rows carrying groups[q][i]), accumulated in f32
        in the order given (one id of weight 1 with one row: that row, bit for bit).  Returns (vectors [B, dim] f32, found
        bool [examples], member_rows int64 [B]); an id no row carries has found False and adds nothing.  d_out: a device
        address that receives the same [B, dim] f32 as well."""
        ids, w, offsets = self._like_args(groups, weights)
        B = offsets.size - 1
        vec = np.zeros((B, self.dim), dtype=np.float32)
        found = np.zeros(max(ids.size, 1), dtype=np.uint8)
        members = np.zeros(max(B, 1), dtype=np.int64)
        _ffi.check(
            _ffi.lib().pcv_searcher_like_queries(
                self._handle, _ffi.i64p(ids) if ids.size else None, _ffi.f32p(w) if w is not None and w.size else None,
                _ffi.i64p(offsets), B, _ffi.f32p(vec) if B else None, C.c_void_p(d_out) if d_out else None, _ffi.u8p(found),
                _ffi.i64p(members),
            )
        )
        return vec, found[: ids.size].astype(bool), members[:B]

    def search_like(self, sources, num_results, groups, weights=None, exclude_examples=True):
        """search_vectors with the vectors like_queries builds, in one call.  exclude_examples: no row carrying one of a
        query's own example ids is a result of that query (the exact top-k of the rest).  Returns (ids [B,k], scores [B,k],
        counts [B], found bool [examples]); a query none of whose examples exists has count 0."""
        ids_in, w, offsets = self._like_args(groups, weights)
        B, k = offsets.size - 1, int(num_results)
        ids = np.full((B, k), -1, dtype=np.int64)
        scores = np.full((B, k), np.nan, dtype=np.float32)
        counts = np.zeros(max(B, 1), dtype=np.int32)
        found = np.zeros(max(ids_in.size, 1), dtype=np.uint8)
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_like(
                self._handle, _ffi.i64p(ids_in) if ids_in.size else None, _ffi.f32p(w) if w is not None and w.size else None,
                _ffi.i64p(offsets), B, src, nsrc, k, 1 if exclude_examples else 0, _ffi.i64p(ids), _ffi.f32p(scores),
                _ffi.i32p(counts), _ffi.u8p(found),
            )
        )
        return ids, scores, counts[:B], found[: ids_in.size].astype(bool)

    def search_like_item(self, sources, num_results, item_id, exclude=False):
        """`perceive search --like <id>` (cmd/search.rs:64-86): search with the stored embedding of `item_id`; as there, the item
        itself is the first hit unless `exclude`.  KeyError("Item not found") when no row carries the id (cmd/search.rs:83)."""
        ids, scores, counts, found = self.search_like(sources, num_results, [[int(item_id)]], exclude_examples=exclude)
        if not found[0]:
            raise KeyError("Item not found")
        return [SearchItem(int(ids[0, j]), float(scores[0, j])) for j in range(int(counts[0]))]

    # ---- range search (pcv_searcher_search_range) ----------------------------------------------------
    # Every item within a score bound instead of the best k: near-duplicates, a "related" list with a quality cut-off.
    def search_range(self, sources, bounds, vectors, max_results):
        """Every searchable row whose reported score passes the bound (cosine: score >= bound; dot: distance <= bound), best
        first, at most max_results per query: vectors [B, dim], bounds [B] or a scalar -> (ids [B, max_results] int64, scores
        [B, max_results] f32, counts [B] int64, more [B] bool: more rows are in range than were returned).  Ids and scores are
        those search_vectors returns for the same rows."""
        q = np.ascontiguousarray(vectors, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"vectors must be [B, {self.dim}]")
        B, m = q.shape[0], int(max_results)
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(bounds, dtype=np.float32), (B,)))
        if not 1 <= m <= (1 << 24):
            raise ValueError("max_results outside [1, 2^24]")
        ids = np.empty((B, m), dtype=np.int64)
        scores = np.empty((B, m), dtype=np.float32)
        counts = np.zeros(max(B, 1), dtype=np.int64)
        more = np.zeros(max(B, 1), dtype=np.uint8)
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_range(
                self._handle, _ffi.f32p(q), B, src, nsrc, _ffi.f32p(b), m, _ffi.i64p(ids), _ffi.f32p(scores), _ffi.i64p(counts),
                _ffi.u8p(more),
            )
        )
        return ids, scores, counts[:B], more[:B].astype(bool)

    def search_range_vector(self, sources, bound, vector, max_results):
        """search_range for one vector -> list[SearchItem] (the `more` flag is dropped: ask search_range for it)."""
        ids, scores, counts, _more = self.search_range(sources, bound, np.asarray(vector, dtype=np.float32)[None, :], max_results)
        return [SearchItem(int(ids[0, j]), float(scores[0, j])) for j in range(int(counts[0]))]

    def search_range_like_item(self, sources, bound, item_id, max_results):
        """The items within `bound` of the stored embedding of `item_id` (like_queries + search_range); as in search_like_item the
        item itself comes first.  KeyError("Item not found") when no row carries the id."""
        vec, found, _members = self.like_queries([[int(item_id)]])
        if not found[0]:
            raise KeyError("Item not found")
        return self.search_range_vector(sources, bound, vec[0], max_results)

    # ---- distinct results (pcv_searcher_search_distinct) ---------------------------------------------
    # The exact top-k with near-duplicates collapsed on the device: the same article under five URLs is one hit.
    def search_distinct(self, sources, num_results, vectors, threshold, pool=None):
        """The ranked list of search_vectors walked best first, a row kept iff its canonical cosine with every row kept before it
        is below `threshold` (in (-1, 1]); at most `pool` entries are examined (default min(PCV_MAX_DISTINCT_POOL, max(128,
        8 * num_results))).  vectors [B, dim] -> (ids [B, k] int64, scores [B, k] f32, counts [B] int32, similar [B, k] int32:
        examined rows dropped in favour of each hit, examined [B] int32, more [B] bool: the walk stopped at `pool` short of
        num_results although the list had more rows).  Ids and scores are those search_vectors returns for the same rows."""
        q = np.ascontiguousarray(vectors, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"vectors must be [B, {self.dim}]")
        B, k = q.shape[0], int(num_results)
        if pool is None:
            pool = min(PCV_MAX_DISTINCT_POOL, max(128, 8 * k))
        ids = np.full((B, max(k, 0)), -1, dtype=np.int64)
        scores = np.full((B, max(k, 0)), np.nan, dtype=np.float32)
        similar = np.zeros((B, max(k, 0)), dtype=np.int32)
        counts = np.zeros(max(B, 1), dtype=np.int32)
        examined = np.zeros(max(B, 1), dtype=np.int32)
        more = np.zeros(max(B, 1), dtype=np.uint8)
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_distinct(
                self._handle, _ffi.f32p(q), B, src, nsrc, k, float(threshold), int(pool), _ffi.i64p(ids), _ffi.f32p(scores),
                _ffi.i32p(counts), _ffi.i32p(similar), _ffi.i32p(examined), _ffi.u8p(more),
            )
        )
        return ids, scores, counts[:B], similar, examined[:B], more[:B].astype(bool)

    def search_distinct_vector(self, sources, num_results, vector, threshold, pool=None):
        """search_distinct for one vector -> list[SearchItem] (the counters are dropped: ask search_distinct for them)."""
        ids, scores, counts, _sim, _ex, _more = self.search_distinct(
            sources, num_results, np.asarray(vector, dtype=np.float32)[None, :], threshold, pool)
        return [SearchItem(int(ids[0, j]), float(scores[0, j])) for j in range(int(counts[0]))]

    def search_distinct_like_item(self, sources, num_results, item_id, threshold, pool=None):
        """Distinct neighbours of the stored embedding of `item_id` (like_queries + search_distinct); as in search_like_item the
        item itself comes first.  KeyError("Item not found") when no row carries the id."""
        vec, found, _members = self.like_queries([[int(item_id)]])
        if not found[0]:
            raise KeyError("Item not found")
        return self.search_distinct_vector(sources, num_results, vec[0], threshold, pool)

    # ---- diverse results (pcv_searcher_search_diverse) -----------------------------------------------
    # Exact greedy maximal marginal relevance on the device: results like this, but not ten versions of the same page.
    def search_diverse(self, sources, num_results, vectors, lam, pool=None):
        """Greedy MMR over the first `pool` entries of the ranked list of search_vectors (default min(PCV_MAX_DIVERSE_POOL,
        max(128, 8 * num_results))): each pick maximises lam * relevance - (1 - lam) * (largest canonical cosine with a row already
        picked), ties to the better rank; lam in [0, 1], 1 = the plain top-k.  vectors [B, dim] -> (ids [B, k] int64 in pick order,
        scores [B, k] f32: those search_vectors returns for the same rows, marginal [B, k] f64: the value each pick was made at,
        ranks [B, k] int32: each pick's place in the ranked list, counts [B] int32, examined [B] int32: entries in the pool,
        exact [B] bool: the picks are provably those of the same walk over the whole list).  The arithmetic is defined in
        include/perceive_hip.h."""
        q = np.ascontiguousarray(vectors, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"vectors must be [B, {self.dim}]")
        B, k = q.shape[0], int(num_results)
        if pool is None:
            pool = min(PCV_MAX_DIVERSE_POOL, max(128, 8 * k))
        ids = np.full((B, max(k, 0)), -1, dtype=np.int64)
        scores = np.full((B, max(k, 0)), np.nan, dtype=np.float32)
        marginal = np.full((B, max(k, 0)), np.nan, dtype=np.float64)
        ranks = np.full((B, max(k, 0)), -1, dtype=np.int32)
        counts = np.zeros(max(B, 1), dtype=np.int32)
        examined = np.zeros(max(B, 1), dtype=np.int32)
        exact = np.zeros(max(B, 1), dtype=np.uint8)
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_diverse(
                self._handle, _ffi.f32p(q), B, src, nsrc, k, float(lam), int(pool), _ffi.i64p(ids), _ffi.f32p(scores),
                _ffi.f64p(marginal), _ffi.i32p(ranks), _ffi.i32p(counts), _ffi.i32p(examined), _ffi.u8p(exact),
            )
        )
        return ids, scores, marginal, ranks, counts[:B], examined[:B], exact[:B].astype(bool)

    def search_diverse_vector(self, sources, num_results, vector, lam, pool=None):
        """search_diverse for one vector -> list[SearchItem] in pick order (the rest is dropped: ask search_diverse for it)."""
        ids, scores, _m, _r, counts, _ex, _exact = self.search_diverse(
            sources, num_results, np.asarray(vector, dtype=np.float32)[None, :], lam, pool)
        return [SearchItem(int(ids[0, j]), float(scores[0, j])) for j in range(int(counts[0]))]

    def search_diverse_like_item(self, sources, num_results, item_id, lam, pool=None):
        """A diverse set of neighbours of the stored embedding of `item_id` (like_queries + search_diverse); as in search_like_item
        the item itself comes first.  KeyError("Item not found") when no row carries the id."""
        vec, found, _members = self.like_queries([[int(item_id)]])
        if not found[0]:
            raise KeyError("Item not found")
        return self.search_diverse_vector(sources, num_results, vec[0], lam, pool)

    # ---- grouped results (pcv_searcher_set_groups / _search_grouped) ---------------------------------
    # The exact top-k collapsed by a stored group key per item: "the k closest documents" over a corpus of chunk rows.
    def set_groups(self, ids, groups):
        """Upsert of the group table: item ids[i] belongs to group groups[i] (any int64 >= 0; PCV_NO_GROUP ungroups the id).  Of an
        id that occurs more than once the last occurrence holds.  Keyed by id: entries survive remove_items, clear_source and
        replace_source.  A view is read-only (PcvError): set the groups on its parent."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).ravel()
        groups = np.ascontiguousarray(groups, dtype=np.int64).ravel()
        if ids.shape != groups.shape:
            raise ValueError("ids and groups must have the same length")
        _ffi.check(_ffi.lib().pcv_searcher_set_groups(self._handle, _ffi.i64p(ids), _ffi.i64p(groups), ids.shape[0]))

    def clear_groups(self):
        """Forget every group: the table is released and its counters start from 0."""
        _ffi.check(_ffi.lib().pcv_searcher_clear_groups(self._handle))

    def groups_of(self, ids):
        """ids [n] -> groups [n] int64, PCV_NO_GROUP for an id without a group (a view answers from its parent's table)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).ravel()
        out = np.full(ids.shape[0], PCV_NO_GROUP, dtype=np.int64)
        _ffi.check(_ffi.lib().pcv_searcher_get_groups(self._handle, _ffi.i64p(ids), ids.shape[0], _ffi.i64p(out)))
        return out

    def group_stats(self):
        """{"ids": ids with a group, "entries": occupied slots, "slots": capacity, "rehashes": growths, "last_set_ms": device time of
        the last set_groups} (pcv_group_stats)."""
        st = _ffi.GroupStats()
        _ffi.check(_ffi.lib().pcv_searcher_group_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.GroupStats._fields_}

    def search_grouped(self, sources, num_results, vectors, pool=None):
        """The ranked list of search_vectors walked best first, a row kept iff no kept row has its group (set_groups; a row without
        a group is a group of its own); at most `pool` entries are examined (default min(PCV_MAX_GROUPED_POOL, max(128,
        8 * num_results))).  vectors [B, dim] -> (ids [B, k] int64, scores [B, k] f32, groups [B, k] int64: PCV_NO_GROUP for a
        row without one, counts [B] int32, collapsed [B, k] int32: examined rows collapsed into each hit, examined [B] int32,
        more [B] bool: the walk stopped at `pool` short of num_results although the list had more rows).  Ids and scores are
        those search_vectors returns for the same rows."""
        q = np.ascontiguousarray(vectors, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"vectors must be [B, {self.dim}]")
        B, k = q.shape[0], int(num_results)
        if pool is None:
            pool = min(PCV_MAX_GROUPED_POOL, max(128, 8 * k))
        ids = np.full((B, max(k, 0)), -1, dtype=np.int64)
        scores = np.full((B, max(k, 0)), np.nan, dtype=np.float32)
        groups = np.full((B, max(k, 0)), PCV_NO_GROUP, dtype=np.int64)
        collapsed = np.zeros((B, max(k, 0)), dtype=np.int32)
        counts = np.zeros(max(B, 1), dtype=np.int32)
        examined = np.zeros(max(B, 1), dtype=np.int32)
        more = np.zeros(max(B, 1), dtype=np.uint8)
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_grouped(
                self._handle, _ffi.f32p(q), B, src, nsrc, k, int(pool), _ffi.i64p(ids), _ffi.f32p(scores), _ffi.i64p(groups),
                _ffi.i32p(counts), _ffi.i32p(collapsed), _ffi.i32p(examined), _ffi.u8p(more),
            )
        )
        return ids, scores, groups, counts[:B], collapsed, examined[:B], more[:B].astype(bool)

    def search_grouped_vector(self, sources, num_results, vector, pool=None):
        """search_grouped for one vector -> list[(SearchItem, group, collapsed)]: the best member of each of the closest groups."""
        ids, scores, groups, counts, collapsed, _ex, _more = self.search_grouped(
            sources, num_results, np.asarray(vector, dtype=np.float32)[None, :], pool)
        return [(SearchItem(int(ids[0, j]), float(scores[0, j])), int(groups[0, j]), int(collapsed[0, j])) for j in range(int(counts[0]))]

    def search_grouped_like_item(self, sources, num_results, item_id, pool=None):
        """The groups closest to the stored embedding of `item_id` (like_queries + search_grouped); as in search_like_item the item
        itself comes first.  KeyError("Item not found") when no row carries the id."""
        vec, found, _members = self.like_queries([[int(item_id)]])
        if not found[0]:
            raise KeyError("Item not found")
        return self.search_grouped_vector(sources, num_results, vec[0], pool)

    # ---- item values and filtered search (pcv_searcher_set_values / _count_where / _search_where / _create_view_where) ----
    # A stored int64 per item and exact search under a range predicate on it: "the best matches among the items modified since ...".
    def set_values(self, ids, values):
        """Upsert of the value table: item ids[i] has value values[i] (any int64; PCV_NO_VALUE unsets the id).  Of an id that occurs
        more than once the last occurrence holds.  Keyed by id: entries survive remove_items, clear_source and replace_source.  A
        view is read-only (PcvError): set the values on its parent."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).ravel()
        values = np.ascontiguousarray(values, dtype=np.int64).ravel()
        if ids.shape != values.shape:
            raise ValueError("ids and values must have the same length")
        _ffi.check(_ffi.lib().pcv_searcher_set_values(self._handle, _ffi.i64p(ids), _ffi.i64p(values), ids.shape[0]))

    def clear_values(self):
        """Forget every value: the table is released and its counters start from 0."""
        _ffi.check(_ffi.lib().pcv_searcher_clear_values(self._handle))

    def values_of(self, ids):
        """ids [n] -> values [n] int64, PCV_NO_VALUE for an id without a value (a view answers from its parent's table)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).ravel()
        out = np.full(ids.shape[0], PCV_NO_VALUE, dtype=np.int64)
        _ffi.check(_ffi.lib().pcv_searcher_get_values(self._handle, _ffi.i64p(ids), ids.shape[0], _ffi.i64p(out)))
        return out

    def value_stats(self):
        """{"ids": ids with a value, "entries": occupied slots, "slots": capacity, "rehashes": growths, "last_set_ms": device time of
        the last set_values} (pcv_value_stats)."""
        st = _ffi.ValueStats()
        _ffi.check(_ffi.lib().pcv_searcher_value_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.ValueStats._fields_}

    @staticmethod
    def _where_flags(unset_passes, outside):
        return (WHERE_UNSET_PASSES if unset_passes else 0) | (WHERE_OUTSIDE if outside else 0)

    def count_where(self, sources, lo, hi, unset_passes=False, outside=False):
        """-> (rows, searchable): the rows of `sources` whose id has a value in [lo, hi] (`outside`: a value not in it; `unset_passes`:
        rows whose id has no value count too), and those of them a search could return (hidden rows left out).  Exact."""
        rows, live = C.c_int64(), C.c_int64()
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(_ffi.lib().pcv_searcher_count_where(self._handle, src, nsrc, int(lo), int(hi), self._where_flags(unset_passes, outside),
                                                       C.byref(rows), C.byref(live)))
        return rows.value, live.value

    def search_where(self, sources, num_results, vectors, lo, hi, unset_passes=False, outside=False, pool=None):
        """The ranked list of search_vectors walked best first, a row kept iff the value of its id passes the predicate (count_where);
        at most `pool` entries are examined (default min(PCV_MAX_WHERE_POOL, max(128, 8 * num_results))).  vectors [B, dim] ->
        (ids [B, k] int64, scores [B, k] f32, values [B, k] int64: PCV_NO_VALUE for an unset row that passed, counts [B] int32,
        examined [B] int32, more [B] bool: the walk stopped at `pool` short of num_results although the list had more rows).  Ids
        and scores are those search_vectors returns for the same rows.  For a predicate few rows pass, use view_where."""
        q = np.ascontiguousarray(vectors, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"vectors must be [B, {self.dim}]")
        B, k = q.shape[0], int(num_results)
        if pool is None:
            pool = min(PCV_MAX_WHERE_POOL, max(128, 8 * k))
        ids = np.full((B, max(k, 0)), -1, dtype=np.int64)
        scores = np.full((B, max(k, 0)), np.nan, dtype=np.float32)
        values = np.full((B, max(k, 0)), PCV_NO_VALUE, dtype=np.int64)
        counts = np.zeros(max(B, 1), dtype=np.int32)
        examined = np.zeros(max(B, 1), dtype=np.int32)
        more = np.zeros(max(B, 1), dtype=np.uint8)
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_where(
                self._handle, _ffi.f32p(q), B, src, nsrc, k, int(pool), int(lo), int(hi), self._where_flags(unset_passes, outside),
                _ffi.i64p(ids), _ffi.f32p(scores), _ffi.i64p(values), _ffi.i32p(counts), _ffi.i32p(examined), _ffi.u8p(more),
            )
        )
        return ids, scores, values, counts[:B], examined[:B], more[:B].astype(bool)

    def search_where_vector(self, sources, num_results, vector, lo, hi, unset_passes=False, outside=False, pool=None):
        """search_where for one vector -> list[(SearchItem, value)]: the best passing rows."""
        ids, scores, values, counts, _ex, _more = self.search_where(
            sources, num_results, np.asarray(vector, dtype=np.float32)[None, :], lo, hi, unset_passes, outside, pool)
        return [(SearchItem(int(ids[0, j]), float(scores[0, j])), int(values[0, j])) for j in range(int(counts[0]))]

    def search_where_like_item(self, sources, num_results, item_id, lo, hi, unset_passes=False, outside=False, pool=None):
        """The passing rows closest to the stored embedding of `item_id` (like_queries + search_where); the item itself comes first if
        it passes.  KeyError("Item not found") when no row carries the id."""
        vec, found, _members = self.like_queries([[int(item_id)]])
        if not found[0]:
            raise KeyError("Item not found")
        return self.search_where_vector(sources, num_results, vec[0], lo, hi, unset_passes, outside, pool)

    def view_where(self, lo, hi, unset_passes=False, outside=False):
        """A read-only searcher over the rows whose id passes the predicate (count_where): a view like view(item_ids) without an id
        list — the rows are selected on the device from the value table, and the view follows every later change of this searcher
        and of its values."""
        h = C.c_void_p()
        _ffi.check(_ffi.lib().pcv_searcher_create_view_where(self._handle, int(lo), int(hi), self._where_flags(unset_passes, outside), C.byref(h)))
        return SearcherView(self, h)

    # ---- boosted results (pcv_searcher_search_boosted) -------------------------------------------------
    # The exact top-k under score plus a prior from the item's value: "the best matches, with recent items ranked a little higher".
    @staticmethod
    def _boost(knot_values, knot_boosts, unset_boost):
        kv = [int(v) for v in np.asarray(knot_values, dtype=object).ravel().tolist()]
        kb = np.asarray(knot_boosts, dtype=np.float64).ravel()
        if len(kv) != kb.shape[0]:
            raise ValueError("knot_values and knot_boosts must have the same length")
        b = _ffi.Boost()
        b.n_knots = len(kv)  # (more than PCV_MAX_BOOST_KNOTS, or none: the library refuses the call)
        for j in range(min(len(kv), PCV_MAX_BOOST_KNOTS)):
            b.knot_values[j] = kv[j]
            b.knot_boosts[j] = float(kb[j])
        b.unset_boost = float(unset_boost)
        return b

    def search_boosted(self, sources, num_results, vectors, knot_values, knot_boosts, unset_boost=0.0, pool=None):
        """The top num_results under m = relevance + boost(value of the item) (set_values), ties to the better rank in the list of
        search_vectors.  boost is piecewise linear through (knot_values[j], knot_boosts[j]) — values strictly increasing, at most
        PCV_MAX_BOOST_KNOTS —, constant beyond both ends, `unset_boost` for an item without a value.  The list is examined
        PCV_MAX_RESULTS entries at a time until the k-th boosted score is out of reach of every row not yet seen, or `pool`
        entries (default min(PCV_MAX_BOOST_POOL, max(128, 8 * num_results))) are examined.  vectors [B, dim] -> (ids [B, k] int64
        best first, scores [B, k] f32: those search_vectors returns for the same rows, boosted [B, k] f64: m, values [B, k] int64:
        PCV_NO_VALUE for an unset row, ranks [B, k] int32: each row's place in the ranked list, counts [B] int32, examined [B]
        int32, exact [B] bool: the rows are provably the top num_results of the whole list).  The arithmetic is defined in
        include/perceive_hip.h."""
        q = np.ascontiguousarray(vectors, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"vectors must be [B, {self.dim}]")
        B, k = q.shape[0], int(num_results)
        if pool is None:
            pool = min(PCV_MAX_BOOST_POOL, max(128, 8 * k))
        boost = self._boost(knot_values, knot_boosts, unset_boost)
        ids = np.full((B, max(k, 0)), -1, dtype=np.int64)
        scores = np.full((B, max(k, 0)), np.nan, dtype=np.float32)
        boosted = np.full((B, max(k, 0)), np.nan, dtype=np.float64)
        values = np.full((B, max(k, 0)), PCV_NO_VALUE, dtype=np.int64)
        ranks = np.full((B, max(k, 0)), -1, dtype=np.int32)
        counts = np.zeros(max(B, 1), dtype=np.int32)
        examined = np.zeros(max(B, 1), dtype=np.int32)
        exact = np.zeros(max(B, 1), dtype=np.uint8)
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_boosted(
                self._handle, _ffi.f32p(q), B, src, nsrc, k, int(pool), C.byref(boost), _ffi.i64p(ids), _ffi.f32p(scores),
                _ffi.f64p(boosted), _ffi.i64p(values), _ffi.i32p(ranks), _ffi.i32p(counts), _ffi.i32p(examined), _ffi.u8p(exact),
            )
        )
        return ids, scores, boosted, values, ranks, counts[:B], examined[:B], exact[:B].astype(bool)

    def search_boosted_vector(self, sources, num_results, vector, knot_values, knot_boosts, unset_boost=0.0, pool=None):
        """search_boosted for one vector -> list[(SearchItem, boosted score, value)], best first."""
        ids, scores, boosted, values, _r, counts, _ex, _exact = self.search_boosted(
            sources, num_results, np.asarray(vector, dtype=np.float32)[None, :], knot_values, knot_boosts, unset_boost, pool)
        return [(SearchItem(int(ids[0, j]), float(scores[0, j])), float(boosted[0, j]), int(values[0, j])) for j in range(int(counts[0]))]

    def search_boosted_like_item(self, sources, num_results, item_id, knot_values, knot_boosts, unset_boost=0.0, pool=None):
        """The boosted neighbours of the stored embedding of `item_id` (like_queries + search_boosted); under a zero boost the item
        itself comes first.  KeyError("Item not found") when no row carries the id."""
        vec, found, _members = self.like_queries([[int(item_id)]])
        if not found[0]:
            raise KeyError("Item not found")
        return self.search_boosted_vector(sources, num_results, vec[0], knot_values, knot_boosts, unset_boost, pool)

    def last_select_stats(self):
        """The select steps of the most recent ranked call (search_distinct, _grouped, _where, _boosted, _diverse, _compound) ->
        (hipEvent ms of their launches, summed; number of launches)."""
        ms, n = C.c_float(0.0), C.c_int32(0)
        _ffi.check(_ffi.lib().pcv_searcher_last_select_stats(self._handle, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- compound queries (pcv_searcher_search_compound / _search_compound_like) ------------------------
    # The exact top-k under "all of these" (min), "any of these" (max) and "but not like that" (a hinge penalty).
    @staticmethod
    def _compound_side(parts, dim):
        """parts: a list of [n_i, dim] arrays (one vector may be given as [dim]), or None -> (vectors f32 [sum n_i, dim],
        offsets int64 [len(parts) + 1]); None -> (None, None)"""
        if parts is None:
            return None, None
        mats = []
        for x in parts:
            m = np.asarray(x, dtype=np.float32)
            m = m.reshape(-1, dim) if m.size else np.zeros((0, dim), dtype=np.float32)
            mats.append(m)
        offsets = np.zeros(len(mats) + 1, dtype=np.int64)
        if mats:
            np.cumsum([m.shape[0] for m in mats], out=offsets[1:])
        vec = np.ascontiguousarray(np.concatenate(mats) if mats else np.zeros((0, dim), dtype=np.float32), dtype=np.float32)
        return vec, offsets

    @staticmethod
    def _compound_mode(mode):
        return COMPOUND_MODES[mode] if mode in COMPOUND_MODES else int(mode)

    @staticmethod
    def _compound_outputs(n, k):
        k0 = max(k, 0)
        return (np.full((n, k0), -1, dtype=np.int64), np.full((n, k0), np.nan, dtype=np.float64),
                np.full((n, k0, PCV_MAX_COMPOUND_PARTS), np.nan, dtype=np.float32), np.full((n, k0), np.nan, dtype=np.float64),
                np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.uint8))

    def search_compound(self, sources, num_results, wants, avoids=None, mode="all", avoid_weight=1.0, pool=None):
        """The top num_results under m = base - avoid_weight * max(0, max_n rel_n): base is the min ("all") or the max ("any") of the
        row's relevance under the compound's wanted vectors, rel_n its relevance under the avoided ones; ties to the lower position.
        wants: a list of [W_i, dim] arrays, one compound each (W_i in 1 .. PCV_MAX_COMPOUND_PARTS); avoids: None, or a list of
        [A_i, dim] arrays of the same length (A_i may be 0).  The W_i ranked lists are walked PCV_MAX_RESULTS entries at a time until
        the k-th kept row beats what any row not yet met can reach, or `pool` entries of each (default
        min(PCV_MAX_COMPOUND_POOL, max(128, 8 * num_results))) are walked.  -> (ids [n, k] int64 best first, combined [n, k] f64: m,
        part_scores [n, k, PCV_MAX_COMPOUND_PARTS] f32: what search_vectors reports for the row under each wanted vector, NaN behind
        W_i, penalties [n, k] f64, counts [n] int32, examined [n] int32, exact [n] bool: the rows are provably the top num_results).
        The arithmetic is defined in include/perceive_hip.h."""
        want, want_off = self._compound_side(wants, self.dim)
        avoid, avoid_off = self._compound_side(avoids, self.dim)
        n, k = want_off.size - 1, int(num_results)
        if avoid_off is not None and avoid_off.size != want_off.size:
            raise ValueError(f"{avoid_off.size - 1} avoid lists for {n} compounds")
        if pool is None:
            pool = min(PCV_MAX_COMPOUND_POOL, max(128, 8 * k))
        ids, combined, parts, penalties, counts, examined, exact = self._compound_outputs(n, k)
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_search_compound(
                self._handle, src, nsrc, k, int(pool), self._compound_mode(mode), float(avoid_weight), _ffi.f32p(want), _ffi.i64p(want_off),
                _ffi.f32p(avoid) if avoid is not None and avoid.size else None, _ffi.i64p(avoid_off) if avoid_off is not None else None, n,
                _ffi.i64p(ids), _ffi.f64p(combined), _ffi.f32p(parts), _ffi.f64p(penalties), _ffi.i32p(counts), _ffi.i32p(examined), _ffi.u8p(exact),
            )
        )
        return ids, combined, parts, penalties, counts[:n], examined[:n], exact[:n].astype(bool)

    @staticmethod
    def _compound_like_side(parts):
        """parts: per compound a list of parts, each part a list of item ids or of (id, weight) pairs; None -> four Nones.
        -> (ids int64, weights f32, example_offsets int64 [parts + 1], offsets int64 [compounds + 1])"""
        if parts is None:
            return None, None, None, None
        ids, weights, ex_off, off = [], [], [0], [0]
        for compound in parts:
            for part in compound:
                for e in part:
                    pair = isinstance(e, (tuple, list))
                    ids.append(int(e[0]) if pair else int(e))
                    weights.append(float(e[1]) if pair else 1.0)
                ex_off.append(len(ids))
            off.append(len(ex_off) - 1)
        return (np.asarray(ids, dtype=np.int64), np.asarray(weights, dtype=np.float32), np.asarray(ex_off, dtype=np.int64),
                np.asarray(off, dtype=np.int64))

    def search_compound_like_items(self, sources, num_results, wants, avoids=None, mode="all", avoid_weight=1.0, pool=None,
                                   exclude_examples=True):
        """search_compound with every vector built on the device from stored items, as like_queries builds them: wants[i] is the list
        of compound i's parts, a part a list of item ids (or (id, weight) pairs) whose rows are summed; avoids likewise or None.
        exclude_examples: no row that carries one of a compound's wanted example ids is in its answer.  Returns what search_compound
        returns."""
        w_ids, w_w, w_ex, w_off = self._compound_like_side(wants)
        a_ids, a_w, a_ex, a_off = self._compound_like_side(avoids)
        n, k = w_off.size - 1, int(num_results)
        if a_off is not None and a_off.size != w_off.size:
            raise ValueError(f"{a_off.size - 1} avoid lists for {n} compounds")
        if pool is None:
            pool = min(PCV_MAX_COMPOUND_POOL, max(128, 8 * k))
        ids, combined, parts, penalties, counts, examined, exact = self._compound_outputs(n, k)
        src, nsrc, _keep = _source_filter(sources)
        ptr = lambda a, f: f(a) if a is not None and a.size else None  # noqa: E731
        _ffi.check(
            _ffi.lib().pcv_searcher_search_compound_like(
                self._handle, src, nsrc, k, int(pool), self._compound_mode(mode), float(avoid_weight), ptr(w_ids, _ffi.i64p), ptr(w_w, _ffi.f32p),
                _ffi.i64p(w_ex), _ffi.i64p(w_off), ptr(a_ids, _ffi.i64p), ptr(a_w, _ffi.f32p), _ffi.i64p(a_ex) if a_ex is not None else None,
                _ffi.i64p(a_off) if a_off is not None else None, n, 1 if exclude_examples else 0, _ffi.i64p(ids), _ffi.f64p(combined),
                _ffi.f32p(parts), _ffi.f64p(penalties), _ffi.i32p(counts), _ffi.i32p(examined), _ffi.u8p(exact),
            )
        )
        return ids, combined, parts, penalties, counts[:n], examined[:n], exact[:n].astype(bool)

    # ---- duplicate pairs (pcv_searcher_find_duplicates) ----------------------------------------------
    # The exact self-join of the corpus: what search_distinct collapses per query, found once for remove_items / hide_items.
    def find_duplicates(self, sources, threshold, max_pairs=1 << 20):
        """Every pair of searchable rows of `sources` whose canonical cosine is >= `threshold` (in (-1, 1]; both metrics), best
        first (ties: lower position of the first row, then of the second), at most max_pairs of them -> (id_a [n] int64, id_b [n]
        int64, scores [n] f32, total): id_a belongs to the row stored first, total is the exact number of pairs (total > n: there
        are more than were returned).  A view joins its own rows."""
        m = int(max_pairs)
        if not 1 <= m <= PCV_MAX_DUPLICATE_PAIRS:
            raise ValueError("max_pairs outside [1, 2^24]")
        id_a = np.empty(m, dtype=np.int64)
        id_b = np.empty(m, dtype=np.int64)
        scores = np.empty(m, dtype=np.float32)
        count, total = C.c_int64(), C.c_int64()
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_find_duplicates(
                self._handle, src, nsrc, float(threshold), m, _ffi.i64p(id_a), _ffi.i64p(id_b), _ffi.f32p(scores), C.byref(count),
                C.byref(total),
            )
        )
        n = count.value
        return id_a[:n].copy(), id_b[:n].copy(), scores[:n].copy(), total.value

    def last_duplicate_stats(self):
        st = _ffi.DuplicateStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_duplicate_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.DuplicateStats._fields_}

    # ---- item labels (pcv_searcher_assign / _label_sums / _kmeans) ----------------------------------
    # The transpose of a search: the best of K vectors for every row, and spherical k-means built on it.
    def _assign_rows(self, src, nsrc):
        n = C.c_int64()
        one = np.zeros((1, self.dim), dtype=np.float32)
        _ffi.check(_ffi.lib().pcv_searcher_assign(self._handle, _ffi.f32p(one), 1, src, nsrc, 0, None, None, None, None, C.byref(n)))
        return n.value

    def assign(self, sources, labels):
        """The best of the K vectors `labels` [K, dim] for every row of `sources`, exact (the canonical score with the label in the
        query's place; ties: the lower label) -> (label [n] int32, score [n] f32 as search reports it, ids [n] int64, counts [K]
        int64), by global position.  A row no search could return has label -1 and a NaN score.  A view assigns its own rows."""
        lab = np.ascontiguousarray(labels, dtype=np.float32)
        if lab.ndim != 2 or lab.shape[1] != self.dim:
            raise ValueError(f"labels must be [K, {self.dim}]")
        K = lab.shape[0]
        src, nsrc, _keep = _source_filter(sources)
        n = self._assign_rows(src, nsrc)
        label = np.empty(max(n, 1), dtype=np.int32)
        score = np.empty(max(n, 1), dtype=np.float32)
        ids = np.empty(max(n, 1), dtype=np.int64)
        counts = np.zeros(max(K, 1), dtype=np.int64)
        got = C.c_int64()
        _ffi.check(
            _ffi.lib().pcv_searcher_assign(
                self._handle, _ffi.f32p(lab), K, src, nsrc, max(n, 1), _ffi.i32p(label), _ffi.f32p(score), _ffi.i64p(ids), _ffi.i64p(counts),
                C.byref(got),
            )
        )
        return label[:n], score[:n], ids[:n], counts[:K]

    def label_sums(self, sources, labels, k):
        """sums [k, dim] int64 of rint(x * rinv * 2^32) over the rows of each label (labels [n] int32 by position as assign returns
        them; negative: none) and the members [k] int64 that went into them: the same bits in any order of addition."""
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        sums = np.zeros((int(k), self.dim), dtype=np.int64)
        members = np.zeros(int(k), dtype=np.int64)
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_label_sums(
                self._handle, src, nsrc, _ffi.i32p(lab) if lab.size else None, lab.size, int(k), _ffi.i64p(sums), _ffi.i64p(members)
            )
        )
        return sums, members

    def kmeans(self, sources, k, init, max_iters=20, seed=0):
        """Spherical k-means by canonical cosine (both metrics), reproducible bit for bit.  init: [k, dim] vectors, or k item ids
        (their stored embeddings, through like_queries), or "kmeans++" / "farthest": the k items seeds(sources, k, init, seed)
        picks (ValueError if it finds fewer than k).  -> (centroids [k, dim] f32 of the last assignment, label [n] int32,
        score [n] f32, ids [n] int64, counts [k] int64, iterations, moved [iterations + 1] int64: rows that changed their label in
        each assignment).  It stops after an assignment that moved no row, or after max_iters updates."""
        if isinstance(init, str):
            picked = self.seeds(sources, k, init, seed)[0]
            if picked.size < int(k):
                raise ValueError(f"kmeans: seeding stopped after {picked.size} of {k} items (no row is left uncovered)")
            init = picked
        init = np.asarray(init)
        if init.ndim == 1:
            if init.size != int(k):
                raise ValueError(f"{init.size} item ids for k = {k}")
            vec, found, _members = self.like_queries([[int(i)] for i in init])
            if not found.all():
                raise ValueError("kmeans: an init item id that no row carries")
            init = vec
        init = np.ascontiguousarray(init, dtype=np.float32)
        if init.shape != (int(k), self.dim):
            raise ValueError(f"init must be [{k}, {self.dim}] vectors or {k} item ids")
        K, iters = int(k), int(max_iters)
        src, nsrc, _keep = _source_filter(sources)
        n = self._assign_rows(src, nsrc)
        cent = np.empty((K, self.dim), dtype=np.float32)
        label = np.empty(max(n, 1), dtype=np.int32)
        score = np.empty(max(n, 1), dtype=np.float32)
        ids = np.empty(max(n, 1), dtype=np.int64)
        counts = np.zeros(K, dtype=np.int64)
        moved = np.zeros(max(iters, 0) + 1, dtype=np.int64)
        done, got = C.c_int32(), C.c_int64()
        _ffi.check(
            _ffi.lib().pcv_searcher_kmeans(
                self._handle, _ffi.f32p(init), K, iters, src, nsrc, max(n, 1), _ffi.f32p(cent), _ffi.i32p(label), _ffi.f32p(score),
                _ffi.i64p(ids), _ffi.i64p(counts), C.byref(done), _ffi.i64p(moved), C.byref(got),
            )
        )
        return cent, label[:n], score[:n], ids[:n], counts, done.value, moved[: done.value + 1].copy()

    def last_assign_stats(self):
        st = _ffi.AssignStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_assign_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.AssignStats._fields_}

    def assign_top(self, sources, labels, m, min_score=None):
        """The m best of the K vectors `labels` [K, dim] for every row of `sources`, exact: the labels j with a defined score
        c >= min_score (None: no bound; under dot a bound on the raw dot product), ordered by (c descending, j ascending) ->
        (labels [n, m] int32 best first with unused slots -1, scores [n, m] f32 as search reports them with unused slots NaN,
        ids [n] int64, counts [n] int32, label_rows [K] int64: rows that list each label), by global position.  With m = 1 and no
        bound: what assign returns.  A view assigns its own rows."""
        lab = np.ascontiguousarray(labels, dtype=np.float32)
        if lab.ndim != 2 or lab.shape[1] != self.dim:
            raise ValueError(f"labels must be [K, {self.dim}]")
        K, m = lab.shape[0], int(m)
        bound = float("-inf") if min_score is None else float(min_score)
        src, nsrc, _keep = _source_filter(sources)
        n = self._assign_rows(src, nsrc)
        room = max(n, 1)
        out = np.empty((room, max(m, 1)), dtype=np.int32)
        score = np.empty((room, max(m, 1)), dtype=np.float32)
        ids = np.empty(room, dtype=np.int64)
        counts = np.zeros(room, dtype=np.int32)
        label_rows = np.zeros(max(K, 1), dtype=np.int64)
        got = C.c_int64()
        _ffi.check(
            _ffi.lib().pcv_searcher_assign_top(
                self._handle, _ffi.f32p(lab), K, m, bound, src, nsrc, room, _ffi.i32p(out), _ffi.f32p(score), _ffi.i64p(ids), _ffi.i32p(counts),
                _ffi.i64p(label_rows), C.byref(got),
            )
        )
        return out[:n], score[:n], ids[:n], counts[:n], label_rows[:K]

    def last_assign_top_stats(self):
        st = _ffi.AssignTopStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_assign_top_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.AssignTopStats._fields_}

    # ---- item neighbours (pcv_searcher_neighbors) --------------------------------------------------
    # The k-nearest-neighbour table of the corpus: what N / 256 search_like calls would give, in one call that no search setting touches.
    def neighbors(self, sources, k):
        """For every row of `sources` its exact k best other rows by canonical cosine (both metrics; ties: the row stored first) ->
        (ids [n] int64, neighbor_ids [n, k] int64, scores [n, k] f32, counts [n] int32), by global position; row i has counts[i]
        neighbours, best first, the unused slots -1 / NaN.  A row no search could return, or without a cosine, has none and is
        nobody's neighbour.  A view lists its own rows."""
        k = int(k)
        if not 1 <= k <= PCV_MAX_NEIGHBORS:
            raise ValueError("k outside [1, %d]" % PCV_MAX_NEIGHBORS)
        src, nsrc, _keep = _source_filter(sources)
        n = C.c_int64()
        _ffi.check(_ffi.lib().pcv_searcher_neighbors(self._handle, src, nsrc, k, 0, None, None, None, None, C.byref(n)))
        n = n.value
        ids = np.empty(max(n, 1), dtype=np.int64)
        nbr = np.empty((max(n, 1), k), dtype=np.int64)
        scores = np.empty((max(n, 1), k), dtype=np.float32)
        counts = np.empty(max(n, 1), dtype=np.int32)
        got = C.c_int64()
        _ffi.check(
            _ffi.lib().pcv_searcher_neighbors(
                self._handle, src, nsrc, k, max(n, 1), _ffi.i64p(ids), _ffi.i64p(nbr), _ffi.f32p(scores), _ffi.i32p(counts), C.byref(got)
            )
        )
        return ids[:n], nbr[:n], scores[:n], counts[:n]

    def last_neighbor_stats(self):
        st = _ffi.NeighborStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_neighbor_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.NeighborStats._fields_}

    # ---- item matches (pcv_searcher_match) -----------------------------------------------------------
    # The join of two sets of sources: `neighbors` with the owners drawn from one selection and the partners from another.
    def match(self, from_sources, to_sources, k, min_score=-1.0):
        """For every row of `from_sources` its exact k best rows of `to_sources` by canonical cosine (both metrics; ties: the row
        stored first) among those with cosine >= min_score (-1.0: no bound) -> (ids [n] int64, match_ids [n, k] int64, scores [n, k]
        f32, counts [n] int32), by global position; row i has counts[i] matches, best first, the unused slots -1 / NaN.  The two
        selections may overlap; a row is never its own match.  match(X, X, k) is neighbors(X, k).  A view matches among its own rows."""
        k = int(k)
        if not 1 <= k <= PCV_MAX_NEIGHBORS:
            raise ValueError("k outside [1, %d]" % PCV_MAX_NEIGHBORS)
        src, nsrc, _keep = _source_filter(from_sources)
        dst, ndst, _keep_to = _source_filter(to_sources)
        lo = float(min_score)
        n = C.c_int64()
        _ffi.check(_ffi.lib().pcv_searcher_match(self._handle, src, nsrc, dst, ndst, k, lo, 0, None, None, None, None, C.byref(n)))
        n = n.value
        ids = np.empty(max(n, 1), dtype=np.int64)
        mids = np.empty((max(n, 1), k), dtype=np.int64)
        scores = np.empty((max(n, 1), k), dtype=np.float32)
        counts = np.empty(max(n, 1), dtype=np.int32)
        got = C.c_int64()
        _ffi.check(
            _ffi.lib().pcv_searcher_match(
                self._handle, src, nsrc, dst, ndst, k, lo, max(n, 1), _ffi.i64p(ids), _ffi.i64p(mids), _ffi.f32p(scores), _ffi.i32p(counts),
                C.byref(got),
            )
        )
        return ids[:n], mids[:n], scores[:n], counts[:n]

    def last_match_stats(self):
        st = _ffi.MatchStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_match_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.MatchStats._fields_}

    # ---- group-aware pairs (pcv_searcher_neighbors_grouped / _match_grouped / _find_duplicates_grouped) ----
    # neighbors, match and find_duplicates over a corpus of chunks: the group table (set_groups) says which rows are one document.
    def neighbors_grouped(self, sources, k, flags=GROUPS_SKIP_OWN):
        """neighbors(sources, k) with the group table consulted -> (ids [n] int64, neighbor_ids [n, k] int64, scores [n, k] f32,
        neighbor_groups [n, k] int64 (NO_GROUP for a singleton and in unused slots), counts [n] int32).  flags: GROUPS_SKIP_OWN —
        the rows of the owner's own group are no partners of it; GROUPS_ONE_PER_GROUP — of every group only its best member is
        kept, the k best groups by best member; both, or 0 for the plain result."""
        k, flags = int(k), int(flags)
        if not 1 <= k <= PCV_MAX_NEIGHBORS:
            raise ValueError("k outside [1, %d]" % PCV_MAX_NEIGHBORS)
        if not 0 <= flags <= 3:
            raise ValueError("flags outside 0..3")
        src, nsrc, _keep = _source_filter(sources)
        n = C.c_int64()
        _ffi.check(_ffi.lib().pcv_searcher_neighbors_grouped(self._handle, src, nsrc, k, flags, 0, None, None, None, None, None, C.byref(n)))
        n = n.value
        ids = np.empty(max(n, 1), dtype=np.int64)
        nbr = np.empty((max(n, 1), k), dtype=np.int64)
        scores = np.empty((max(n, 1), k), dtype=np.float32)
        groups = np.empty((max(n, 1), k), dtype=np.int64)
        counts = np.empty(max(n, 1), dtype=np.int32)
        got = C.c_int64()
        _ffi.check(
            _ffi.lib().pcv_searcher_neighbors_grouped(
                self._handle, src, nsrc, k, flags, max(n, 1), _ffi.i64p(ids), _ffi.i64p(nbr), _ffi.f32p(scores), _ffi.i64p(groups),
                _ffi.i32p(counts), C.byref(got),
            )
        )
        return ids[:n], nbr[:n], scores[:n], groups[:n], counts[:n]

    def match_grouped(self, from_sources, to_sources, k, min_score=-1.0, flags=GROUPS_SKIP_OWN):
        """match(from_sources, to_sources, k, min_score) with the group table consulted, as neighbors_grouped does -> (ids [n]
        int64, match_ids [n, k] int64, scores [n, k] f32, match_groups [n, k] int64, counts [n] int32)."""
        k, flags = int(k), int(flags)
        if not 1 <= k <= PCV_MAX_NEIGHBORS:
            raise ValueError("k outside [1, %d]" % PCV_MAX_NEIGHBORS)
        if not 0 <= flags <= 3:
            raise ValueError("flags outside 0..3")
        src, nsrc, _keep = _source_filter(from_sources)
        dst, ndst, _keep_to = _source_filter(to_sources)
        lo = float(min_score)
        n = C.c_int64()
        _ffi.check(_ffi.lib().pcv_searcher_match_grouped(self._handle, src, nsrc, dst, ndst, k, lo, flags, 0, None, None, None, None, None, C.byref(n)))
        n = n.value
        ids = np.empty(max(n, 1), dtype=np.int64)
        mids = np.empty((max(n, 1), k), dtype=np.int64)
        scores = np.empty((max(n, 1), k), dtype=np.float32)
        groups = np.empty((max(n, 1), k), dtype=np.int64)
        counts = np.empty(max(n, 1), dtype=np.int32)
        got = C.c_int64()
        _ffi.check(
            _ffi.lib().pcv_searcher_match_grouped(
                self._handle, src, nsrc, dst, ndst, k, lo, flags, max(n, 1), _ffi.i64p(ids), _ffi.i64p(mids), _ffi.f32p(scores),
                _ffi.i64p(groups), _ffi.i32p(counts), C.byref(got),
            )
        )
        return ids[:n], mids[:n], scores[:n], groups[:n], counts[:n]

    def find_duplicates_grouped(self, sources, threshold, max_pairs=1 << 20):
        """find_duplicates(sources, threshold, max_pairs) without the pairs of rows of one group -> (id_a [n] int64, id_b [n]
        int64, scores [n] f32, total, skipped): total counts the pairs of non-siblings, skipped the sibling pairs at or above the
        threshold, which find_duplicates would report."""
        m = int(max_pairs)
        if not 1 <= m <= PCV_MAX_DUPLICATE_PAIRS:
            raise ValueError("max_pairs outside [1, 2^24]")
        id_a = np.empty(m, dtype=np.int64)
        id_b = np.empty(m, dtype=np.int64)
        scores = np.empty(m, dtype=np.float32)
        count, total, skipped = C.c_int64(), C.c_int64(), C.c_int64()
        src, nsrc, _keep = _source_filter(sources)
        _ffi.check(
            _ffi.lib().pcv_searcher_find_duplicates_grouped(
                self._handle, src, nsrc, float(threshold), m, _ffi.i64p(id_a), _ffi.i64p(id_b), _ffi.f32p(scores), C.byref(count),
                C.byref(total), C.byref(skipped),
            )
        )
        n = count.value
        return id_a[:n].copy(), id_b[:n].copy(), scores[:n].copy(), total.value, skipped.value

    def last_pair_group_stats(self):
        st = _ffi.PairGroupStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_pair_group_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.PairGroupStats._fields_}

    # ---- density clusters (pcv_searcher_density_clusters) -------------------------------------------
    # DBSCAN under the canonical cosine: the clusters, their number and the noise, with no number of groups to choose.
    def density_clusters(self, sources, threshold, min_items):
        """Two rows are near iff their canonical cosine is >= threshold (both metrics); a row with min_items - 1 near rows or more
        is a core row; clusters are the connected components of the core rows, numbered by their first core row; a row near a core
        row takes the label of the one stored first (a border row); the rest is noise.  -> (ids [n] int64, labels [n] int32: -1 for
        noise and for rows that take no part, kinds [n] int8: PCV_DENSITY_CORE / _BORDER / _NOISE / _NONE, degrees [n] int32: the
        near rows of each row, n_clusters), by global position.  A view clusters its own rows."""
        threshold, min_items = float(threshold), int(min_items)
        if not -1.0 < threshold <= 1.0:
            raise ValueError("threshold outside (-1, 1]")
        if min_items < 1:
            raise ValueError("min_items below 1")
        src, nsrc, _keep = _source_filter(sources)
        n = C.c_int64()
        _ffi.check(_ffi.lib().pcv_searcher_density_clusters(self._handle, src, nsrc, threshold, min_items, 0, None, None, None, None, C.byref(n), None))
        n = n.value
        ids = np.empty(max(n, 1), dtype=np.int64)
        labels = np.empty(max(n, 1), dtype=np.int32)
        kinds = np.empty(max(n, 1), dtype=np.int8)
        degrees = np.empty(max(n, 1), dtype=np.int32)
        got, clusters = C.c_int64(), C.c_int32()
        _ffi.check(
            _ffi.lib().pcv_searcher_density_clusters(
                self._handle, src, nsrc, threshold, min_items, max(n, 1), _ffi.i64p(ids), _ffi.i32p(labels),
                _ffi.i8p(kinds), _ffi.i32p(degrees), C.byref(got), C.byref(clusters),
            )
        )
        return ids[:n], labels[:n], kinds[:n], degrees[:n], clusters.value

    def last_density_stats(self):
        st = _ffi.DensityStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_density_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.DensityStats._fields_}

    # ---- linkage tree (pcv_searcher_linkage_tree) ---------------------------------------------------
    # The single-linkage hierarchy: the clusters of the corpus at every threshold at once (linkage_cut cuts it).
    def linkage_tree(self, sources):
        """The maximum spanning tree of the participating rows of `sources` under the canonical cosine (both metrics), edges ordered
        by (c descending, lower position, higher position): the single-linkage merge order -> (ids [n] int64, part [n] int8: 1 iff
        the row takes part, pos_a [e] int64, pos_b [e] int64: positions into ids with pos_a < pos_b, id_a [e], id_b [e] int64,
        c [e] float64), e = participating rows - 1 (or 0).  A view uses its own rows."""
        src, nsrc, _keep = _source_filter(sources)
        n = C.c_int64()
        _ffi.check(_ffi.lib().pcv_searcher_linkage_tree(self._handle, src, nsrc, 0, None, None, None, None, None, None, None, C.byref(n), None))
        n = n.value
        cap = max(n, 1)
        ids = np.empty(cap, dtype=np.int64)
        part = np.empty(cap, dtype=np.int8)
        pos_a, pos_b, id_a, id_b = (np.empty(cap, dtype=np.int64) for _ in range(4))
        c = np.empty(cap, dtype=np.float64)
        got, edges = C.c_int64(), C.c_int64()
        _ffi.check(
            _ffi.lib().pcv_searcher_linkage_tree(
                self._handle, src, nsrc, cap, _ffi.i64p(ids), _ffi.i8p(part), _ffi.i64p(pos_a), _ffi.i64p(pos_b), _ffi.i64p(id_a),
                _ffi.i64p(id_b), _ffi.f64p(c), C.byref(got), C.byref(edges),
            )
        )
        e = edges.value
        return ids[:n], part[:n], pos_a[:e], pos_b[:e], id_a[:e], id_b[:e], c[:e]

    def last_linkage_stats(self):
        st = _ffi.LinkageStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_linkage_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.LinkageStats._fields_}

    # ---- reach tree (pcv_searcher_reach_tree) -------------------------------------------------------
    # The spanning tree under the mutual-reachability weight: what HDBSCAN starts from (linkage_select picks the clusters).
    def reach_tree(self, sources, min_items):
        """The spanning tree of the participating rows of `sources` under w(a, b) = min(core(a), core(b), c(a, b)), core(r) the
        (min_items - 1)-th largest canonical cosine of r with another participating row (+inf for min_items = 1), edges ordered by
        (w descending, lower position, higher position) -> (ids [n] int64, part [n] int8, core [n] float64: NaN where part == 0,
        pos_a [e], pos_b [e], id_a [e], id_b [e] int64, w [e] float64, c [e] float64), e = participating rows - 1 (or 0).  With
        min_items = 1 it is linkage_tree's output (w == c).  A view uses its own rows."""
        src, nsrc, _keep = _source_filter(sources)
        n = C.c_int64()
        lib = _ffi.lib()
        _ffi.check(
            lib.pcv_searcher_reach_tree(self._handle, src, nsrc, int(min_items), 0, None, None, None, None, None, None, None, None, None, C.byref(n), None)
        )
        n = n.value
        cap = max(n, 1)
        ids = np.empty(cap, dtype=np.int64)
        part = np.empty(cap, dtype=np.int8)
        core = np.empty(cap, dtype=np.float64)
        pos_a, pos_b, id_a, id_b = (np.empty(cap, dtype=np.int64) for _ in range(4))
        w = np.empty(cap, dtype=np.float64)
        c = np.empty(cap, dtype=np.float64)
        got, edges = C.c_int64(), C.c_int64()
        _ffi.check(
            lib.pcv_searcher_reach_tree(
                self._handle, src, nsrc, int(min_items), cap, _ffi.i64p(ids), _ffi.i8p(part), _ffi.f64p(core), _ffi.i64p(pos_a), _ffi.i64p(pos_b),
                _ffi.i64p(id_a), _ffi.i64p(id_b), _ffi.f64p(w), _ffi.f64p(c), C.byref(got), C.byref(edges),
            )
        )
        e = edges.value
        return ids[:n], part[:n], core[:n], pos_a[:e], pos_b[:e], id_a[:e], id_b[:e], w[:e], c[:e]

    def last_reach_stats(self):
        st = _ffi.ReachStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_reach_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.ReachStats._fields_}

    # ---- seed items (pcv_searcher_seeds) ------------------------------------------------------------
    # k items that cover the corpus, picked one after the other on the device: the init of kmeans, or a representative sample.
    def seeds(self, sources, k, method="kmeans++", seed=0, first_id=None):
        """k seed items of `sources`: "kmeans++" draws each with probability proportional to its integer weight rint((1 - largest
        canonical cosine with a seed so far) * 2^32) (seed_draw(seed, step, total)); "farthest" takes the largest weight (ties: the
        row stored first).  first_id: the item step 0 picks instead.  -> (ids [n] int64, positions [n] int64, totals [n] int64: the
        potential before each pick in units of 2^-32, cover [n] f32: the pick's largest cosine with the seeds before it, NaN at
        step 0), n <= k: the picks stop when no row is left uncovered.  A view seeds its own rows."""
        k = int(k)
        if not 1 <= k <= PCV_MAX_SEEDS:
            raise ValueError("k outside [1, %d]" % PCV_MAX_SEEDS)
        if method not in _SEED_METHODS:
            raise ValueError('method must be "kmeans++" or "farthest"')
        src, nsrc, _keep = _source_filter(sources)
        ids = np.empty(k, dtype=np.int64)
        pos = np.empty(k, dtype=np.int64)
        totals = np.empty(k, dtype=np.int64)
        cover = np.empty(k, dtype=np.float32)
        first = None if first_id is None else np.array([int(first_id)], dtype=np.int64)
        count = C.c_int32()
        _ffi.check(
            _ffi.lib().pcv_searcher_seeds(
                self._handle, src, nsrc, k, _SEED_METHODS[method], int(seed) & 0xFFFFFFFFFFFFFFFF, None if first is None else _ffi.i64p(first),
                _ffi.i64p(ids), _ffi.i64p(pos), _ffi.i64p(totals), _ffi.f32p(cover), C.byref(count),
            )
        )
        n = count.value
        return ids[:n].copy(), pos[:n].copy(), totals[:n].copy(), cover[:n].copy()

    def last_seed_stats(self):
        st = _ffi.SeedStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_seed_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.SeedStats._fields_}

    # ---- corpus moments and principal axes (pcv_searcher_moments / _principal_axes / _project) -----
    # A PCA where the rows live: integer moments of the unit rows, a Jacobi solve on the host, every row's coordinates.
    def moments(self, sources, centered=False, matrix=True):
        """The integer moments of the unit rows of `sources` -> (sums [dim] int64: S_d = sum of t(r, d) = rint(x * rinv * 2^32), matrix
        [dim, dim] f64 or None, n: the participating rows).  With C = T^T T in exact integers the matrix is C * 2^-64 (n times the
        second moment), or with centered (n C - S S^T) * 2^-64 (n^2 times the covariance), rounded once.  matrix=False: the sums alone."""
        src, nsrc, _keep = _source_filter(sources)
        sums = np.zeros(self.dim, dtype=np.int64)
        mat = np.zeros((self.dim, self.dim), dtype=np.float64) if matrix else None
        n = C.c_int64()
        _ffi.check(
            _ffi.lib().pcv_searcher_moments(self._handle, src, nsrc, 1 if centered else 0, _ffi.i64p(sums), None if mat is None else mat.ctypes.data, C.byref(n))
        )
        return sums, mat, n.value

    def last_moment_stats(self):
        st = _ffi.MomentStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_moment_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.MomentStats._fields_}

    def principal_axes(self, sources, m):
        """The m leading principal axes of the unit rows of `sources` -> (axes [m, dim] f32, offsets [m] f64: the mean unit row along
        each axis, what project subtracts, variance [m] f64 along each axis, n: the participating rows)."""
        m = int(m)
        if not 1 <= m <= PCV_MAX_AXES:
            raise ValueError("m outside [1, %d]" % PCV_MAX_AXES)
        src, nsrc, _keep = _source_filter(sources)
        axes = np.zeros((m, self.dim), dtype=np.float32)
        offsets = np.zeros(m, dtype=np.float64)
        variance = np.zeros(m, dtype=np.float64)
        n = C.c_int64()
        _ffi.check(
            _ffi.lib().pcv_searcher_principal_axes(self._handle, src, nsrc, m, _ffi.f32p(axes), offsets.ctypes.data, variance.ctypes.data, C.byref(n))
        )
        return axes, offsets, variance, n.value

    def project(self, sources, axes, offsets=None):
        """coord(r, j) = (float)(canonical f64 dot(axes[j], row r) * rinv_r - offsets[j]) for every row of `sources` and every axis
        (axes [m, dim] f32, offsets [m] f64 or None: zeros) -> (coords [n, m] f32, ids [n] int64), by global position; a row that
        takes no part has NaN in all m slots."""
        ax = np.ascontiguousarray(axes, dtype=np.float32)
        if ax.ndim != 2 or ax.shape[1] != self.dim:
            raise ValueError(f"axes must be [m, {self.dim}]")
        m = ax.shape[0]
        if not 1 <= m <= PCV_MAX_AXES:
            raise ValueError("m outside [1, %d]" % PCV_MAX_AXES)
        off = None
        if offsets is not None:
            off = np.ascontiguousarray(offsets, dtype=np.float64)
            if off.shape != (m,):
                raise ValueError(f"offsets must be [{m}]")
        src, nsrc, _keep = _source_filter(sources)
        n = C.c_int64()
        poff = None if off is None else off.ctypes.data
        _ffi.check(_ffi.lib().pcv_searcher_project(self._handle, _ffi.f32p(ax), poff, m, src, nsrc, 0, None, None, C.byref(n)))
        n = n.value
        coords = np.empty((max(n, 1), m), dtype=np.float32)
        ids = np.empty(max(n, 1), dtype=np.int64)
        got = C.c_int64()
        _ffi.check(
            _ffi.lib().pcv_searcher_project(self._handle, _ffi.f32p(ax), poff, m, src, nsrc, max(n, 1), _ffi.f32p(coords), _ffi.i64p(ids), C.byref(got))
        )
        return coords[:n], ids[:n]

    def last_project_stats(self):
        st = _ffi.ProjectStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_project_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.ProjectStats._fields_}

    # ---- introspection ------------------------------------------------------------------------
    def set_kernel(self, kernel="auto"):
        _ffi.check(_ffi.lib().pcv_searcher_set_kernel(self._handle, _KERNELS[kernel]))

    def allow_wide_sharded_pass(self, on=True):
        """Every rank's searcher keeps the int8 copy of all its rows (the host has checked): a pass among ranks may take 256
        queries (pcv_searcher_allow_wide_sharded_pass)."""
        _ffi.check(_ffi.lib().pcv_searcher_allow_wide_sharded_pass(self._handle, 1 if on else 0))

    def wait_background(self):
        """Wait for a mid copy that AUTO is building beside the searches (pcv_searcher_wait_background)."""
        _ffi.check(_ffi.lib().pcv_searcher_wait_background(self._handle))

    def set_candidate_capacity(self, n_candidates):
        """Initial rows per query of a pass's candidate lists (tuning; a pass that needs more repeats itself)."""
        _ffi.check(_ffi.lib().pcv_searcher_set_candidate_capacity(self._handle, int(n_candidates)))

    def set_tuning(self, flags=0, fail_copy_alloc=False):
        """Diagnostic / comparison switches (pcv_searcher_set_tuning): `flags` as PCV_SCAN_FLAGS (csrc/scan.h), e.g. 32 = no
        speculative start threshold; fail_copy_alloc: screening-copy allocations fail while set (tests)."""
        _ffi.check(_ffi.lib().pcv_searcher_set_tuning(self._handle, (int(flags) & 0xBFFFFFFF) | ((1 << 30) if fail_copy_alloc else 0)))

    def set_screening_copy(self, mode="auto"):
        """"off" | "bf16" | "int8" | "auto" (= int8): keep a narrow copy of the scaled rows next to the f32 rows so that
        the coarse screen streams a half / a quarter of the bytes (pcv_searcher_set_screening_copy); built at the next
        finalize.  Results do not depend on it."""
        _ffi.check(_ffi.lib().pcv_searcher_set_screening_copy(self._handle, {"off": 0, "bf16": 1, "on": 1, "auto": 2, "int8": 3}[mode]))

    def set_mid_copy(self, mode="auto"):
        """"off" | "auto" | "on": the row-major 16-bit copy the fine screen reads in front of the f32 rows
        (pcv_searcher_set_mid_copy); results do not depend on it."""
        _ffi.check(_ffi.lib().pcv_searcher_set_mid_copy(self._handle, {"off": 0, "auto": 1, "on": 2}[mode]))

    def set_shard_offset(self, first_global_pos):
        _ffi.check(_ffi.lib().pcv_searcher_set_shard_offset(self._handle, int(first_global_pos)))

    @property
    def num_rows(self):
        n = C.c_int64()
        _ffi.check(_ffi.lib().pcv_searcher_num_rows(self._handle, C.byref(n)))
        return n.value

    @property
    def num_segments(self):
        n = C.c_int()
        _ffi.check(_ffi.lib().pcv_searcher_num_segments(self._handle, C.byref(n)))
        return n.value

    @property
    def source_ids(self):
        n = C.c_int()
        _ffi.check(_ffi.lib().pcv_searcher_num_sources(self._handle, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int64)
        _ffi.check(_ffi.lib().pcv_searcher_source_ids(self._handle, _ffi.i64p(out), out.size))
        return [int(x) for x in out[: n.value]]

    def source_num_rows(self, source_id):
        n = C.c_int64()
        _ffi.check(_ffi.lib().pcv_searcher_source_num_rows(self._handle, int(source_id), C.byref(n)))
        return n.value

    def get_rows(self, positions):
        pos = np.ascontiguousarray(positions, dtype=np.int64)
        rows = np.empty((pos.size, self.dim), dtype=np.float32)
        ids = np.empty(pos.size, dtype=np.int64)
        _ffi.check(_ffi.lib().pcv_searcher_get_rows(self._handle, _ffi.i64p(pos), pos.size, _ffi.f32p(rows), _ffi.i64p(ids)))
        return rows, ids

    # ---- hidden items (pcv_searcher_hide_ids) -------------------------------------------------------
    # Unlike `self.hidden` above, these are consulted: rows carrying a hidden id are no result of any search until they are
    # unhidden, without a rebuild.  The set persists across finalize / rebuild_source; rows keep their positions.
    def hide_items(self, ids):
        """Hide every row carrying one of `ids` (int64 1-D array or iterable); returns the rows that were hidden by it."""
        return self._hide_call(_ffi.lib().pcv_searcher_hide_ids, ids)

    def unhide_items(self, ids):
        """Return the rows carrying one of `ids` to the results (exactly as before); returns the rows that came back."""
        return self._hide_call(_ffi.lib().pcv_searcher_unhide_ids, ids)

    def hidden_items(self):
        """The hidden set, ascending (int64 array)."""
        n = C.c_int64()
        _ffi.check(_ffi.lib().pcv_searcher_hidden_ids(self._handle, None, 0, C.byref(n), None))
        out = np.zeros(max(n.value, 1), dtype=np.int64)
        _ffi.check(_ffi.lib().pcv_searcher_hidden_ids(self._handle, _ffi.i64p(out), out.size, C.byref(n), None))
        return out[: n.value]

    @property
    def hidden_rows(self):
        """Rows hidden now."""
        n, rows = C.c_int64(), C.c_int64()
        _ffi.check(_ffi.lib().pcv_searcher_hidden_ids(self._handle, None, 0, C.byref(n), C.byref(rows)))
        return rows.value

    def _hide_call(self, fn, ids):
        a = np.ascontiguousarray(ids if isinstance(ids, np.ndarray) else np.fromiter(ids, dtype=np.int64), dtype=np.int64)
        if a.ndim != 1:
            raise ValueError("ids must be 1-D")
        rows = C.c_int64()
        _ffi.check(fn(self._handle, _ffi.i64p(a) if a.size else None, a.size, C.byref(rows)))
        return rows.value

    # ---- removed items (pcv_searcher_remove_ids) ----------------------------------------------------
    # An item that is gone for good leaves the device: its rows are dropped and the rows behind them move down, without a rebuild
    # or an upload; searches afterwards return what a searcher built fresh from the remaining rows returns.  Positions shift.
    def remove_items(self, ids):
        """Remove every row carrying one of `ids` (int64 1-D array or iterable; duplicates and unknown ids allowed), in every
        source; returns the rows removed.  Needs a finalized searcher.  The ids are not remembered (unlike hide_items)."""
        return self._hide_call(_ffi.lib().pcv_searcher_remove_ids, ids)

    # ---- updated items (pcv_searcher_update_rows) ---------------------------------------------------
    # A re-embedded item takes its new vector in place, in every row carrying its id, without a rebuild; searches afterwards return
    # what a searcher built fresh from the updated rows returns.
    def update_items(self, ids, rows):
        """Rows carrying ids[i] take rows[i] ([n, dim] f32).  Returns (found: bool [n], rows_changed); ids no row carries change
        nothing.  Needs a finalized searcher; duplicate ids are refused."""
        ids = self._update_ids(ids)
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.shape != (ids.size, self.dim):
            raise ValueError(f"rows must be [{ids.size}, {self.dim}]")
        return self._update_call(_ffi.lib().pcv_searcher_update_rows, ids, _ffi.f32p(rows) if ids.size else None)

    def update_blobs(self, ids, blobs: bytes, n):
        """update_items with the vectors as n embedding blobs of dim*4 bytes (serialize_embedding), as add_blobs takes them."""
        ids = self._update_ids(ids)
        b = np.frombuffer(blobs, dtype=np.uint8)
        if ids.size != n or b.size != n * self.dim * 4:
            raise ValueError("ids / blob bytes do not match n, n*dim*4")
        return self._update_call(_ffi.lib().pcv_searcher_update_blobs, ids, _ffi.u8p(b) if n else None)

    def upsert_items(self, source_id, ids, rows):
        """What a source scan produces (update_db.rs upserts New / Changed embeddings): ids some row carries take their new vector
        in place, the others are added to `source_id`; then finalize.  Returns (rows_replaced, rows_appended)."""
        ids = self._update_ids(ids)
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        found, replaced = self.update_items(ids, rows)
        new = ~found
        if new.any():
            self.add_rows(source_id, rows[new], ids[new])
        self.finalize()
        return replaced, int(new.sum())

    @staticmethod
    def _update_ids(ids):
        a = np.ascontiguousarray(ids if isinstance(ids, np.ndarray) else np.fromiter(ids, dtype=np.int64), dtype=np.int64)
        if a.ndim != 1:
            raise ValueError("ids must be 1-D")
        return a

    def _update_call(self, fn, ids, rows_p):
        found = np.zeros(max(ids.size, 1), dtype=np.uint8)
        n = C.c_int64()
        _ffi.check(fn(self._handle, _ffi.i64p(ids) if ids.size else None, rows_p, ids.size, _ffi.u8p(found), C.byref(n)))
        return found[: ids.size].astype(bool), n.value

    def last_stats(self):
        st = _ffi.ScanStats()
        _ffi.check(_ffi.lib().pcv_searcher_last_stats(self._handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ffi.ScanStats._fields_}

    # ---- views (pcv_searcher_create_view) -----------------------------------------------------------
    def view(self, item_ids):
        """A read-only searcher over the rows carrying one of `item_ids` (int64 1-D array or iterable; duplicates and unknown ids
        allowed): it searches like a searcher built fresh from only those rows, in this searcher's source and row order, with its
        hidden set applied, and follows every later change of this searcher.  Device hit lists carry this searcher's positions."""
        a = self._update_ids(item_ids)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().pcv_searcher_create_view(self._handle, _ffi.i64p(a) if a.size else None, a.size, C.byref(h)))
        return SearcherView(self, h)

    @property
    def _handle(self):
        if not self._h:
            raise RuntimeError("searcher already closed")
        return self._h

    def close(self):
        if self._h:
            for v in list(getattr(self, "_views", ())):  # (the library refuses to destroy a searcher whose views are alive)
                v.close()
            if self.ctx._h:  # a context that is gone took its handles with it
                _ffi.lib().pcv_searcher_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SearcherView(Searcher):
    """Searcher.view(item_ids): every search of Searcher (search_vector(s), search_device, the begin / end and sharded searches,
    like_queries / search_like / search_like_item with the examples looked up in the parent), last_stats, num_rows,
    source_ids, source_num_rows and the kernel / tuning settings; what would change rows or copies raises PcvError
    (status 1), as get_rows does.  Close it before its parent (the parent's close closes it)."""

    def __init__(self, parent, handle):
        self.ctx, self.dim, self.metric = parent.ctx, parent.dim, parent.metric
        self.parent = parent
        self._h = handle
        self.hidden = set()
        if not hasattr(parent, "_views"):
            parent._views = weakref.WeakSet()
        parent._views.add(self)
        self.ctx._register(self)

    def view_stats(self):
        """{"rows": rows held now, "ids": distinct allowed ids, "refreshes": copies made again since the parent changed,
        "build_ms": device time of the last copy}"""
        rows, ids, ref, ms = C.c_int64(), C.c_int64(), C.c_int32(), C.c_float()
        _ffi.check(_ffi.lib().pcv_searcher_view_stats(self._handle, C.byref(rows), C.byref(ids), C.byref(ref), C.byref(ms)))
        return {"rows": rows.value, "ids": ids.value, "refreshes": ref.value, "build_ms": ms.value}

    def view(self, item_ids):
        raise _ffi.PcvError(1, "a view cannot be the parent of a view")

    def view_where(self, lo, hi, unset_passes=False, outside=False):
        raise _ffi.PcvError(1, "a view cannot be the parent of a view")

    def close(self):
        if self._h:
            if self.ctx._h:
                _ffi.lib().pcv_searcher_destroy(self._h)
            self._h = C.c_void_p()


def duplicate_groups(id_a, id_b):
    """Groups of duplicates from the pairs of find_duplicates (host only) -> (ids [n] int64: the distinct ids of the pairs,
    ascending; group [n] int64: the smallest id of each one's connected component).  ids[group != ids] are the items to remove to
    keep one of every group."""
    a = np.ascontiguousarray(id_a, dtype=np.int64).reshape(-1)
    b = np.ascontiguousarray(id_b, dtype=np.int64).reshape(-1)
    if a.size != b.size:
        raise ValueError("id_a and id_b differ in length")
    cap = max(1, 2 * a.size)
    ids = np.empty(cap, dtype=np.int64)
    group = np.empty(cap, dtype=np.int64)
    n = C.c_int64()
    _ffi.check(
        _ffi.lib().pcv_duplicate_groups(
            _ffi.i64p(a) if a.size else None, _ffi.i64p(b) if b.size else None, a.size, _ffi.i64p(ids), _ffi.i64p(group), cap, C.byref(n)
        )
    )
    return ids[: n.value].copy(), group[: n.value].copy()


def linkage_cut(pos_a, pos_b, c, n_rows, part=None, threshold=-np.inf, min_clusters=1):
    """Cuts the tree of Searcher.linkage_tree (host only): edge i is kept iff c[i] >= threshold and i < len(c) - (min_clusters - 1)
    -> (labels [n_rows] int32: the components of the kept edges, numbered by their lowest position, -1 where part == 0; the number
    of clusters).  threshold t alone gives the components of the graph c >= t; min_clusters K alone gives K clusters."""
    a = np.ascontiguousarray(pos_a, dtype=np.int64).reshape(-1)
    b = np.ascontiguousarray(pos_b, dtype=np.int64).reshape(-1)
    cc = np.ascontiguousarray(c, dtype=np.float64).reshape(-1)
    if not a.size == b.size == cc.size:
        raise ValueError("pos_a, pos_b and c differ in length")
    n_rows = int(n_rows)
    pt = None if part is None else np.ascontiguousarray(part, dtype=np.int8).reshape(-1)
    if pt is not None and pt.size != n_rows:
        raise ValueError("part has not n_rows entries")
    labels = np.empty(max(n_rows, 1), dtype=np.int32)
    clusters = C.c_int32()
    _ffi.check(
        _ffi.lib().pcv_linkage_cut(
            _ffi.i64p(a) if a.size else None, _ffi.i64p(b) if a.size else None, _ffi.f64p(cc) if a.size else None, a.size,
            _ffi.i8p(pt) if pt is not None and pt.size else None, n_rows, float(threshold), int(min_clusters), _ffi.i32p(labels), C.byref(clusters),
        )
    )
    return labels[:n_rows].copy(), clusters.value


def linkage_select(pos_a, pos_b, w, n_rows, part=None, min_cluster_size=5, allow_single=False):
    """Picks clusters from the tree of Searcher.reach_tree (or linkage_tree, with its c) without a threshold (host only): HDBSCAN's
    condensed tree with min_cluster_size and excess-of-mass selection, the cosine itself as the density level -> (labels [n_rows]
    int32: the selected clusters numbered by the lowest position of their rows, -1 for noise and where part == 0; stability [k]
    float64; size [k] int64)."""
    a = np.ascontiguousarray(pos_a, dtype=np.int64).reshape(-1)
    b = np.ascontiguousarray(pos_b, dtype=np.int64).reshape(-1)
    ww = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    if not a.size == b.size == ww.size:
        raise ValueError("pos_a, pos_b and w differ in length")
    n_rows = int(n_rows)
    pt = None if part is None else np.ascontiguousarray(part, dtype=np.int8).reshape(-1)
    if pt is not None and pt.size != n_rows:
        raise ValueError("part has not n_rows entries")
    labels = np.empty(max(n_rows, 1), dtype=np.int32)
    cap = max(n_rows // max(int(min_cluster_size), 1), 1)  # (selected clusters are disjoint and hold min_cluster_size rows, but for the root)
    stability = np.empty(cap, dtype=np.float64)
    size = np.empty(cap, dtype=np.int64)
    clusters = C.c_int32()
    _ffi.check(
        _ffi.lib().pcv_linkage_select(
            _ffi.i64p(a) if a.size else None, _ffi.i64p(b) if a.size else None, _ffi.f64p(ww) if a.size else None, a.size,
            _ffi.i8p(pt) if pt is not None and pt.size else None, n_rows, int(min_cluster_size), 1 if allow_single else 0, _ffi.i32p(labels),
            C.byref(clusters), _ffi.f64p(stability), _ffi.i64p(size), cap,
        )
    )
    k = clusters.value
    return labels[:n_rows].copy(), stability[:k].copy(), size[:k].copy()


def seed_draw(seed, step, total):
    """The draw of step `step` of Searcher.seeds among `total` units of weight (host only): floor(z * total / 2^64), z the
    splitmix64 finaliser of seed + (step + 1) * 0x9E3779B97F4A7C15.  The device calls the same function."""
    t = C.c_uint64()
    _ffi.check(_ffi.lib().pcv_seed_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(total), C.byref(t)))
    return t.value


def symmetric_eigen(a):
    """Eigenvalues (descending) and unit eigenvectors (rows; the component of largest magnitude positive) of the symmetric matrix `a`
    [n, n] f64, read from its upper triangle, by cyclic Jacobi on the host (pcv_symmetric_eigen): an offline call, seconds at n = 384."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError("a must be [n, n]")
    n = a.shape[0]
    values = np.zeros(n, dtype=np.float64)
    vectors = np.zeros((n, n), dtype=np.float64)
    _ffi.check(_ffi.lib().pcv_symmetric_eigen(a.ctypes.data, n, values.ctypes.data, vectors.ctypes.data))
    return values, vectors


def encode_query(model, query):
    """search.rs:262-264"""
    return np.asarray(model.encode([query]))[0]


def merge_topk(ctx, metric, dim, d_lists, n_shards, n_queries, k, flagged=False):
    """Cross-shard merge of all-gathered per-shard lists (device pointer) -> (ids, scores, counts);
    flagged=True: lists made by search_device_begin (one overflow record per shard), returns
    (ids, scores, counts, any_overflow)."""
    ids = np.full((n_queries, k), -1, dtype=np.int64)
    scores = np.full((n_queries, k), np.nan, dtype=np.float32)
    counts = np.zeros(n_queries, dtype=np.int32)
    args = (
        ctx.handle, _METRICS[metric], int(dim), C.c_void_p(d_lists), int(n_shards), int(n_queries), int(k),
        _ffi.i64p(ids), _ffi.f32p(scores), _ffi.i32p(counts),
    )
    if flagged:
        over = C.c_int()
        _ffi.check(_ffi.lib().pcv_merge_topk_flagged(*args, C.byref(over)))
        return ids, scores, counts, bool(over.value)
    _ffi.check(_ffi.lib().pcv_merge_topk(*args))
    return ids, scores, counts


# ---- lib.rs:63-77 -----------------------------------------------------------------------------
def _sim(ctx, a, m, cosine):
    a = np.ascontiguousarray(a, dtype=np.float32)
    m = np.ascontiguousarray(m, dtype=np.float32)
    out = np.empty((a.shape[0], m.shape[0]), dtype=np.float32)
    fn = _ffi.lib().pcv_cosine_similarity if cosine else _ffi.lib().pcv_dot_product
    _ffi.check(fn(ctx.handle, _ffi.f32p(a), a.shape[0], _ffi.f32p(m), m.shape[0], a.shape[1], _ffi.f32p(out)))
    return out


def dot_product(ctx, set1, set2):
    """lib.rs:63-65: set1.matmul(set2.T) -> [len(set1), len(set2)]"""
    return _sim(ctx, set1, set2, False)


def cosine_similarity_single_query(ctx, query, matches):
    """lib.rs:67-71: query [D], matches [N, D] -> [N]"""
    return _sim(ctx, np.asarray(query, dtype=np.float32)[None, :], matches, True)[0]


def cosine_similarity_multi_query(ctx, set1, set2):
    """lib.rs:73-77"""
    return _sim(ctx, set1, set2, True)
