// searcher.cpp — the C entry points of the Searcher (replaces search.rs:29-260 of the reference): each checks its arguments,
// takes s->mu and hands over to the unit that does the work — searcher_store.cpp (rows and copies), searcher_edits.cpp (changes
// by id), searcher_views.cpp, searcher_calls.cpp (the search calls) over searcher_pass.cpp (the pass pipeline).  The sharded
// search and the merge calls are in searcher_exchange.cpp, the calls over the stored rows themselves in row_jobs.cpp.
//
// A searcher owns, per source, a list of device-resident corpus segments in the blocked HBM layout
// (scan.h).  Searching streams the selected segments once; see scan_kernels.hip for the pipeline.
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iterator>
#include <numeric>

#include "searcher_calls.h"

using namespace pcv;

namespace {

// A view is read-only: every call that would change its rows or copies is refused.
inline void refuse_view(const pcv_searcher* s, const char* who) {
    PCV_REQUIRE(s->view_parent == nullptr, "%s: the searcher is a view (read-only): change its parent instead", who);
}

// What hide, unhide, remove and update ask before they change a row (s->mu held).
void begin_change(const pcv_searcher* s, const char* who) {
    refuse_view(s, who);
    PCV_REQUIRE(!s->dirty, "%s: pending rows; call pcv_searcher_finalize first", who);
    PCV_REQUIRE(!s->pending.active, "%s: a queued pass has not been collected", who);
}

// What the ranked calls (distinct, grouped, diverse) ask of their arguments; `pool_max`: the call's PCV_MAX_*_POOL.
void check_ranked_args(const pcv_searcher* s, const float* queries, int n_queries, int num_results, int pool, const char* who, int pool_max) {
    PCV_REQUIRE(s != nullptr, "%s: searcher is NULL", who);
    PCV_REQUIRE(queries != nullptr && n_queries > 0, "%s: no queries", who);
    PCV_REQUIRE(num_results >= 1 && num_results <= (int)PCV_MAX_RESULTS, "%s: num_results %d outside [1,%d]", who, num_results,
                (int)PCV_MAX_RESULTS);
    PCV_REQUIRE(pool >= num_results && pool <= pool_max, "%s: pool %d outside [num_results = %d, %d]", who, pool, num_results, pool_max);
}

}  // namespace

extern "C" {

pcv_status pcv_searcher_create(pcv_ctx* ctx, int dim, int metric, pcv_searcher** out) {
    return guarded([&] {
        PCV_REQUIRE(ctx != nullptr && out != nullptr, "searcher_create: NULL argument");
        *out = nullptr;
        PCV_REQUIRE(dim > 0 && dim <= 8192, "searcher_create: dim %d outside [1,8192]", dim);
        PCV_REQUIRE(metric == PCV_METRIC_COSINE || metric == PCV_METRIC_DOT, "searcher_create: unknown metric %d",
                    metric);
        PCV_HIP(hipSetDevice(ctx->device));
        auto s = std::make_unique<pcv_searcher>();
        s->ctx = ctx;
        s->D = dim;
        s->Dp = (dim + 63) / 64 * 64;
        s->D4 = s->Dp / 4;
        s->metric = metric;
        if (const char* f = getenv("PCV_SCAN_FLAGS")) s->scan_flags = (uint32_t)strtoul(f, nullptr, 0);
        if (getenv("PCV_NO_SCAN_GRAPH")) s->use_graph = false;
        if (const char* f = getenv("PCV_SCREEN_COPY")) {  // 0 off, 1 on, 2 auto
            const int mode = atoi(f);
            if (mode >= PCV_SCREEN_COPY_OFF && mode <= PCV_SCREEN_COPY_INT8) s->screen_copy = mode;
        }
        PCV_HIP(hipMalloc((void**)&s->d_max_norm_bits, 4));
        // on the stream the row_scales atomics will run on (the context stream does not wait for the null stream)
        hipError_t e = hipMemsetAsync(s->d_max_norm_bits, 0, 4, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(s->d_max_norm_bits);
            PCV_FAIL(PCV_ERR_DEVICE, "searcher_create: %s", hipGetErrorString(e));
        }
        *out = s.release();
    });
}

namespace {
// everything a searcher (or a view) holds; a view lets go of its parent
void destroy_searcher(pcv_searcher* s) {
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    try {
        settle_mid_build(s, true);
    } catch (...) {
    }
    if (s->side) {
        (void)hipStreamSynchronize(s->side);
        (void)hipStreamDestroy(s->side);
        (void)hipEventDestroy(s->side_go);
        (void)hipEventDestroy(s->mid_done);
    }
    for (auto& src : s->sources)
        for (auto& g : src.segs) free_segment(g);
    for (pcv_searcher::IdTable* t : {&s->groups, &s->values}) {
        if (t->keys) (void)hipFree(t->keys);
        if (t->vals) (void)hipFree(t->vals);
    }
    if (s->graph_exec) (void)hipGraphExecDestroy(s->graph_exec);
    if (s->d_max_norm_bits) (void)hipFree(s->d_max_norm_bits);
    for (auto& e : s->ev)
        if (e) (void)hipEventDestroy(e);
    if (s->view_parent) s->view_parent->live_views.fetch_sub(1);
    delete s;  // (with every DevBuf and PinBuf of it)
}
}  // namespace

pcv_status pcv_searcher_destroy(pcv_searcher* s) {
    return guarded([&] {
        if (!s) return;
        PCV_REQUIRE(s->live_views.load() == 0, "searcher_destroy: %d view(s) of this searcher are alive; destroy them first",
                    s->live_views.load());
        destroy_searcher(s);
    });
}

namespace {
// What both kinds of view are made by (parent->mu held, the arguments checked): `setup` gives the fresh handle its allow list or its
// predicate, then the rows are copied.
pcv_searcher* make_view(pcv_searcher* parent, const char* who, const std::function<void(pcv_searcher*)>& setup) {
    PCV_REQUIRE(!parent->dirty, "%s: pending rows; call pcv_searcher_finalize first", who);
    PCV_REQUIRE(!parent->pending.active, "%s: a queued pass has not been collected", who);
    PCV_HIP(hipSetDevice(parent->ctx->device));
    pcv_searcher* v = new pcv_searcher();
    v->ctx = parent->ctx;
    v->D = parent->D;
    v->Dp = parent->Dp;
    v->D4 = parent->D4;
    v->metric = parent->metric;
    v->kernel = parent->kernel;
    v->scan_flags = parent->scan_flags;
    v->cand_cap = parent->cand_cap;
    v->use_graph = parent->use_graph;
    setup(v);
    v->view_parent = parent;
    parent->live_views.fetch_add(1);  // (given back by destroy_searcher, also if the build fails)
    try {
        build_view(v, parent);
    } catch (...) {
        destroy_searcher(v);
        throw;
    }
    return v;
}

// The predicate of the filtered calls: any flag bit but the two known ones is refused.
WherePred check_where(int64_t lo, int64_t hi, uint32_t flags, const char* who) {
    PCV_REQUIRE((flags & ~(uint32_t)(PCV_WHERE_UNSET_PASSES | PCV_WHERE_OUTSIDE)) == 0, "%s: unknown flag bits in %#x", who, flags);
    return WherePred{lo, hi, flags};
}
}  // namespace

pcv_status pcv_searcher_create_view(pcv_searcher* parent, const int64_t* ids, int64_t n, pcv_searcher** out_view) {
    return guarded([&] {
        PCV_REQUIRE(parent != nullptr && out_view != nullptr, "create_view: NULL argument");
        *out_view = nullptr;
        PCV_REQUIRE(n >= 0 && (ids != nullptr || n == 0), "create_view: bad id list (NULL with n > 0, or n < 0)");
        PCV_REQUIRE(parent->view_parent == nullptr, "create_view: the parent is itself a view");
        std::vector<int64_t> allow(ids, ids + n);
        std::sort(allow.begin(), allow.end());
        allow.erase(std::unique(allow.begin(), allow.end()), allow.end());
        std::lock_guard<std::mutex> lk(parent->mu);
        *out_view = make_view(parent, "create_view", [&](pcv_searcher* v) { v->view_ids.swap(allow); });
    });
}

pcv_status pcv_searcher_create_view_where(pcv_searcher* parent, int64_t lo, int64_t hi, uint32_t flags, pcv_searcher** out_view) {
    return guarded([&] {
        PCV_REQUIRE(parent != nullptr && out_view != nullptr, "create_view_where: NULL argument");
        *out_view = nullptr;
        const WherePred w = check_where(lo, hi, flags, "create_view_where");
        PCV_REQUIRE(parent->view_parent == nullptr, "create_view_where: the parent is itself a view");
        std::lock_guard<std::mutex> lk(parent->mu);
        *out_view = make_view(parent, "create_view_where", [&](pcv_searcher* v) {
            v->view_by_value = true;
            v->view_where = w;
        });
    });
}

pcv_status pcv_searcher_view_stats(pcv_searcher* v, int64_t* out_rows, int64_t* out_ids, int32_t* out_refreshes, float* out_build_ms) {
    return guarded([&] {
        PCV_REQUIRE(v != nullptr, "view_stats: searcher is NULL");
        PCV_REQUIRE(v->view_parent != nullptr, "view_stats: the searcher is not a view");
        std::lock_guard<std::mutex> lk(v->mu);
        PCV_REQUIRE(!v->pending.active, "view_stats: a queued pass has not been collected");
        sync_view(v);
        if (out_rows) *out_rows = v->view_rows;
        if (out_ids) *out_ids = (int64_t)v->view_ids.size();  // (0 for a predicate view: it stores no list)
        if (out_refreshes) *out_refreshes = v->view_refreshes;
        if (out_build_ms) *out_build_ms = v->view_build_ms;
    });
}

pcv_status pcv_searcher_reserve(pcv_searcher* s, int64_t source_id, int64_t n_rows) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "reserve: searcher is NULL");
        refuse_view(s, "reserve");
        PCV_REQUIRE(n_rows >= 0, "reserve: negative row count");
        std::lock_guard<std::mutex> lk(s->mu);
        Source& src = s->get_or_add_source(source_id);
        src.reserve = src.rows() + n_rows;
    });
}

pcv_status pcv_searcher_add_rows(pcv_searcher* s, int64_t source_id, const int64_t* ids, const float* rows,
                                 int64_t n) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "add_rows: searcher is NULL");
        refuse_view(s, "add_rows");
        PCV_REQUIRE(n >= 0 && (rows != nullptr || n == 0), "add_rows: bad rows/n");
        std::lock_guard<std::mutex> lk(s->mu);
        Source& src = s->get_or_add_source(source_id);
        if (n == 0) return;
        PCV_HIP(hipSetDevice(s->ctx->device));
        append_rows(s, src, ids, rows, n);
    });
}

pcv_status pcv_searcher_add_blobs(pcv_searcher* s, int64_t source_id, const int64_t* ids, const uint8_t* blobs,
                                  int64_t n) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "add_blobs: searcher is NULL");
        refuse_view(s, "add_blobs");
        PCV_REQUIRE(n >= 0 && (blobs != nullptr || n == 0), "add_blobs: bad blobs/n");
        // deserialize_embedding (search.rs:281-286) reads little-endian f32; this library only runs on
        // little-endian hosts (x86-64 + gfx950), where that is the identity on the bytes
        const uint32_t probe = 1;
        PCV_REQUIRE(*reinterpret_cast<const uint8_t*>(&probe) == 1, "add_blobs: big-endian host");
        std::lock_guard<std::mutex> lk(s->mu);
        Source& src = s->get_or_add_source(source_id);
        if (n == 0) return;
        PCV_HIP(hipSetDevice(s->ctx->device));
        append_rows(s, src, ids, blobs, n);
    });
}

static pcv_status add_synthetic(pcv_searcher* s, int64_t source_id, int64_t n, uint64_t seed, int64_t first_row,
                                int normalize, int n_clusters, float noise, float amp_lo = 0.0f, float amp_hi = 0.0f) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "add_synthetic: searcher is NULL");
        refuse_view(s, "add_synthetic");
        PCV_REQUIRE(n >= 0, "add_synthetic: negative row count");
        PCV_REQUIRE(n_clusters >= 0 && noise >= 0.0f && std::isfinite(noise), "add_synthetic: bad cluster shape");
        PCV_REQUIRE(std::isfinite(amp_lo) && std::isfinite(amp_hi) && amp_lo >= 0.0f && amp_hi >= amp_lo, "add_synthetic: bad amplitude range");
        PCV_REQUIRE(s->D % 4 == 0, "add_synthetic: dim %d is not a multiple of 4", s->D);
        std::lock_guard<std::mutex> lk(s->mu);
        Source& src = s->get_or_add_source(source_id);
        if (n == 0) return;
        PCV_HIP(hipSetDevice(s->ctx->device));
        hipStream_t st = s->ctx->stream;
        // one segment per <= 2^31 rows, generated in place
        const int64_t kMaxRows = (int64_t)1 << 31;
        for (int64_t r0 = 0; r0 < n; r0 += kMaxRows) {
            const int64_t m = std::min(kMaxRows, n - r0);
            Segment g = alloc_segment(s, m, false);
            g.id0 = first_row + r0;
            try {
                launch_synth_fill(st, g.blk, (uint32_t)m, 0, s->D, s->D4, seed, first_row + r0, normalize,
                                  (uint32_t)n_clusters, noise, amp_lo, amp_hi);
                PCV_HIP(hipStreamSynchronize(st));
                PCV_HIP(hipGetLastError());
            } catch (...) {
                free_segment(g);
                throw;
            }
            g.nrows = (uint32_t)m;
            src.segs.push_back(g);
            s->dirty = true;
        }
    });
}

pcv_status pcv_searcher_add_synthetic(pcv_searcher* s, int64_t source_id, int64_t n, uint64_t seed,
                                      int64_t first_row, int normalize) {
    return add_synthetic(s, source_id, n, seed, first_row, normalize, 0, 0.0f);
}

pcv_status pcv_searcher_add_synthetic_clustered(pcv_searcher* s, int64_t source_id, int64_t n, uint64_t seed,
                                                int64_t first_row, int normalize, int n_clusters, float noise) {
    return add_synthetic(s, source_id, n, seed, first_row, normalize, n_clusters, noise);
}

pcv_status pcv_searcher_add_synthetic_scaled(pcv_searcher* s, int64_t source_id, int64_t n, uint64_t seed,
                                             int64_t first_row, float amp_lo, float amp_hi) {
    if (!(amp_hi > amp_lo) || !(amp_lo > 0.0f)) {
        set_error("add_synthetic_scaled: amplitudes must satisfy 0 < amp_lo < amp_hi");
        return PCV_ERR_INVALID;
    }
    return add_synthetic(s, source_id, n, seed, first_row, 0, 0, 0.0f, amp_lo, amp_hi);
}

pcv_status pcv_searcher_clear_source(pcv_searcher* s, int64_t source_id) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "clear_source: searcher is NULL");
        refuse_view(s, "clear_source");
        std::lock_guard<std::mutex> lk(s->mu);
        Source* src = s->find_source(source_id);
        if (!src) return;
        PCV_HIP(hipSetDevice(s->ctx->device));
        PCV_HIP(hipStreamSynchronize(s->ctx->stream));
        settle_mid_build(s, true);
        if (!src->segs.empty()) s->screen_copy_gave_way = s->mid_gave_way = s->six_gave_way = false;  // rows are given back: AUTO may try its copies again
        for (auto& g : src->segs) free_segment(g);
        src->segs.clear();
        src->next_implicit_id = 0;
        src->reserve = 0;
        s->dirty = true;
        s->gen += 1;
    });
}

pcv_status pcv_searcher_replace_source(pcv_searcher* s, int64_t from_source_id, int64_t to_source_id) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "replace_source: searcher is NULL");
        refuse_view(s, "replace_source");
        PCV_REQUIRE(from_source_id != to_source_id, "replace_source: a source cannot replace itself");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "replace_source: a queued pass has not been collected");
        PCV_HIP(hipSetDevice(s->ctx->device));
        PCV_HIP(hipStreamSynchronize(s->ctx->stream));
        settle_mid_build(s, true);
        std::vector<Segment> fresh;
        int64_t next_id = 0;
        for (size_t i = 0; i < s->sources.size(); ++i)
            if (s->sources[i].id == from_source_id) {
                fresh = std::move(s->sources[i].segs);
                next_id = s->sources[i].next_implicit_id;
                s->sources.erase(s->sources.begin() + (std::ptrdiff_t)i);
                break;
            }
        Source* to = s->find_source(to_source_id);
        if (!to && !fresh.empty()) to = &s->get_or_add_source(to_source_id);
        if (to) {  // (the old rows keep their place among the sources: positions of the others do not move)
            // The staged rebuild holds the old and the new rows of a source at once.  If AUTO gave its copies up to fit them
            // (alloc_segment: the rows come first), the old rows going now is the room to have them again: the next finalize
            // tries — once; another failure gives them up again.  (Without this every later search of a searcher that once
            // rebuilt a large source on a nearly full device streamed the f32 rows, 4x the bytes, silently.)
            if (!to->segs.empty()) s->screen_copy_gave_way = s->mid_gave_way = s->six_gave_way = false;
            for (auto& g : to->segs) free_segment(g);
            to->segs = std::move(fresh);
            to->next_implicit_id = next_id;
            to->reserve = 0;
        }
        s->dirty = true;  // positions are handed out again by finalize (an emptied source disappears there)
        s->gen += 1;
    });
}

pcv_status pcv_searcher_finalize(pcv_searcher* s) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "finalize: searcher is NULL");
        refuse_view(s, "finalize");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_HIP(hipSetDevice(s->ctx->device));
        do_finalize(s);
    });
}

static pcv_status hide_or_unhide(pcv_searcher* s, const int64_t* ids, int64_t n, int64_t* out_rows, bool hide) {
    const char* who = hide ? "hide_ids" : "unhide_ids";
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "%s: searcher is NULL", who);
        PCV_REQUIRE(n >= 0 && (ids != nullptr || n == 0), "%s: bad id list", who);
        std::lock_guard<std::mutex> lk(s->mu);
        begin_change(s, who);
        if (out_rows) *out_rows = 0;
        // the batch: the ids whose membership changes, ascending and distinct
        std::vector<int64_t> batch(ids, ids + n);
        std::sort(batch.begin(), batch.end());
        batch.erase(std::unique(batch.begin(), batch.end()), batch.end());
        std::vector<int64_t> batch_in;  // ... of it, the ones in the set
        std::set_intersection(batch.begin(), batch.end(), s->hidden.begin(), s->hidden.end(), std::back_inserter(batch_in));
        std::vector<int64_t> next;
        if (hide) {
            std::vector<int64_t> fresh;
            std::set_difference(batch.begin(), batch.end(), batch_in.begin(), batch_in.end(), std::back_inserter(fresh));
            batch.swap(fresh);
            std::set_union(s->hidden.begin(), s->hidden.end(), batch.begin(), batch.end(), std::back_inserter(next));
        } else {
            batch.swap(batch_in);
            std::set_difference(s->hidden.begin(), s->hidden.end(), batch.begin(), batch.end(), std::back_inserter(next));
        }
        if (batch.empty()) return;
        PCV_HIP(hipSetDevice(s->ctx->device));
        settle_mid_build(s, true);  // (the AUTO mid build reads the scales and writes the mid copy)
        const int64_t changed = apply_id_batch(s, batch, hide);
        s->hidden.swap(next);
        s->gen += 1;
        if (out_rows) *out_rows = changed;
    });
}

pcv_status pcv_searcher_hide_ids(pcv_searcher* s, const int64_t* ids, int64_t n, int64_t* out_rows) {
    return hide_or_unhide(s, ids, n, out_rows, true);
}

pcv_status pcv_searcher_unhide_ids(pcv_searcher* s, const int64_t* ids, int64_t n, int64_t* out_rows) {
    return hide_or_unhide(s, ids, n, out_rows, false);
}

pcv_status pcv_searcher_remove_ids(pcv_searcher* s, const int64_t* ids, int64_t n, int64_t* out_rows) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "remove_ids: searcher is NULL");
        PCV_REQUIRE(n >= 0 && (ids != nullptr || n == 0), "remove_ids: bad id list (NULL with n > 0, or n < 0)");
        std::lock_guard<std::mutex> lk(s->mu);
        begin_change(s, "remove_ids");
        if (out_rows) *out_rows = 0;
        if (n == 0) return;
        std::vector<int64_t> batch(ids, ids + n);
        std::sort(batch.begin(), batch.end());
        batch.erase(std::unique(batch.begin(), batch.end()), batch.end());
        PCV_HIP(hipSetDevice(s->ctx->device));
        PCV_HIP(hipStreamSynchronize(s->ctx->stream));
        settle_mid_build(s, true);  // (the AUTO mid build reads the rows and scales and writes the mid copy)
        drop_pass_graph(s);
        const int64_t removed = remove_by_id(s, batch);
        refresh_copy_state(s);
        s->gen += 1;  // (views copy their rows again at their next call)
        if (out_rows) *out_rows = removed;
    });
}

pcv_status pcv_searcher_hidden_ids(pcv_searcher* s, int64_t* out_ids, int64_t cap, int64_t* out_n, int64_t* out_hidden_rows) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out_n != nullptr, "hidden_ids: NULL argument");
        PCV_REQUIRE(cap >= 0 && (out_ids != nullptr || cap == 0), "hidden_ids: bad output buffer");
        std::lock_guard<std::mutex> lk(s->mu);
        *out_n = (int64_t)s->hidden.size();
        std::copy_n(s->hidden.begin(), (size_t)std::min<int64_t>(cap, *out_n), out_ids);
        if (out_hidden_rows) {
            int64_t rows = 0;
            for (const auto& src : s->sources)
                for (const auto& g : src.segs) rows += g.hidden_rows;
            *out_hidden_rows = rows;
        }
    });
}

static pcv_status update_call(pcv_searcher* s, const int64_t* ids, const void* rows, int64_t n, uint8_t* out_found, int64_t* out_rows,
                              const char* who) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "%s: searcher is NULL", who);
        PCV_REQUIRE(n >= 0 && ((ids != nullptr && rows != nullptr) || n == 0), "%s: bad ids/rows/n (NULL with n > 0, or n < 0)", who);
        PCV_REQUIRE(n <= 0x7fffffff, "%s: %lld ids in one call", who, (long long)n);
        const uint32_t probe = 1;  // (blobs: little-endian f32, as pcv_searcher_add_blobs reads them)
        PCV_REQUIRE(*reinterpret_cast<const uint8_t*>(&probe) == 1, "%s: big-endian host", who);
        std::lock_guard<std::mutex> lk(s->mu);
        begin_change(s, who);
        if (out_rows) *out_rows = 0;
        if (out_found && n > 0) std::memset(out_found, 0, (size_t)n);
        if (n == 0) return;
        std::vector<uint32_t> by_id(n);  // slots ascending by id: no id twice
        std::iota(by_id.begin(), by_id.end(), 0u);
        std::sort(by_id.begin(), by_id.end(), [&](uint32_t a, uint32_t b) { return ids[a] < ids[b]; });
        for (int64_t i = 1; i < n; ++i)
            PCV_REQUIRE(ids[by_id[i - 1]] != ids[by_id[i]], "%s: id %lld appears twice in the batch", who, (long long)ids[by_id[i]]);
        PCV_HIP(hipSetDevice(s->ctx->device));
        settle_mid_build(s, true);  // (the AUTO mid build reads the rows and scales and writes the mid copy)
        std::vector<uint8_t> found((size_t)n, 0);
        const auto stage_back = at_exit([s] { s->d_stage.release(); });  // whatever happens (as finalize gives it back)
        const int64_t changed = update_by_id(s, ids, rows, n, by_id, found);
        if (changed) s->gen += 1;
        if (out_found) std::memcpy(out_found, found.data(), (size_t)n);
        if (out_rows) *out_rows = changed;
    });
}

pcv_status pcv_searcher_update_rows(pcv_searcher* s, const int64_t* ids, const float* rows, int64_t n, uint8_t* out_found,
                                    int64_t* out_rows) {
    return update_call(s, ids, rows, n, out_found, out_rows, "update_rows");
}

pcv_status pcv_searcher_update_blobs(pcv_searcher* s, const int64_t* ids, const uint8_t* blobs, int64_t n, uint8_t* out_found,
                                     int64_t* out_rows) {
    return update_call(s, ids, blobs, n, out_found, out_rows, "update_blobs");
}

pcv_status pcv_searcher_dim(pcv_searcher* s, int* out_dim) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out_dim != nullptr, "searcher_dim: NULL argument");
        *out_dim = s->D;
    });
}

pcv_status pcv_searcher_num_rows(pcv_searcher* s, int64_t* out_rows) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out_rows != nullptr, "num_rows: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        sync_view(s);
        int64_t n = 0;
        for (auto& src : s->sources)
            if (src.id != PCV_STAGING_SOURCE) n += src.rows();  // (staged rows are not the searcher's rows yet)
        *out_rows = n;
    });
}

pcv_status pcv_searcher_num_segments(pcv_searcher* s, int* out_n) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out_n != nullptr, "num_segments: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        sync_view(s);
        int n = 0;
        for (auto& src : s->sources) n += (int)src.segs.size();
        *out_n = n;
    });
}

pcv_status pcv_searcher_num_sources(pcv_searcher* s, int* out_n) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out_n != nullptr, "num_sources: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        sync_view(s);
        int n = 0;
        for (const auto& src : s->sources) n += src.id != PCV_STAGING_SOURCE ? 1 : 0;
        *out_n = n;
    });
}

pcv_status pcv_searcher_source_ids(pcv_searcher* s, int64_t* out_ids, int cap) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out_ids != nullptr, "source_ids: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        sync_view(s);
        size_t n = 0;
        for (const auto& src : s->sources) n += src.id != PCV_STAGING_SOURCE ? 1 : 0;
        PCV_REQUIRE(cap >= (int)n, "source_ids: capacity %d < %zu sources", cap, n);
        n = 0;
        for (const auto& src : s->sources)
            if (src.id != PCV_STAGING_SOURCE) out_ids[n++] = src.id;
    });
}

pcv_status pcv_searcher_source_num_rows(pcv_searcher* s, int64_t source_id, int64_t* out_rows) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out_rows != nullptr, "source_num_rows: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        sync_view(s);
        PCV_REQUIRE(!s->dirty, "source_num_rows: pending rows; call pcv_searcher_finalize first");
        *out_rows = 0;
        if (Source* src = s->find_source(source_id)) *out_rows = src->rows();
    });
}

pcv_status pcv_searcher_get_rows(pcv_searcher* s, const int64_t* positions, int64_t n, float* out_rows,
                                 int64_t* out_ids) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && positions != nullptr && out_rows != nullptr && n >= 0, "get_rows: bad argument");
        refuse_view(s, "get_rows");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->dirty, "get_rows: pending rows; call pcv_searcher_finalize first");
        if (n == 0) return;
        PCV_HIP(hipSetDevice(s->ctx->device));
        hipStream_t st = s->ctx->stream;
        std::vector<SegDesc> segs;
        for (auto& src : s->sources)
            for (auto& g : src.segs)
                segs.push_back(SegDesc{g.blk, g.scale, g.ids, g.id0, g.pos0, g.nrows, g.nblocks(), 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr});
        DevBuf<SegDesc> d_segs;
        DevBuf<int64_t> d_pos, d_ids;
        DevBuf<float> d_rows;
        d_segs.ensure(segs.size() + 1);
        d_pos.ensure(n);
        d_ids.ensure(n);
        d_rows.ensure((size_t)n * s->D);
        PCV_HIP(hipMemcpyAsync(d_segs.p, segs.data(), segs.size() * sizeof(SegDesc), hipMemcpyHostToDevice, st));
        PCV_HIP(hipMemcpyAsync(d_pos.p, positions, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
        launch_gather_rows(st, d_segs.p, (int)segs.size(), d_pos.p, n, s->D, s->D4, d_rows.p, d_ids.p);
        PCV_HIP(hipMemcpyAsync(out_rows, d_rows.p, (size_t)n * s->D * sizeof(float), hipMemcpyDeviceToHost, st));
        if (out_ids) PCV_HIP(hipMemcpyAsync(out_ids, d_ids.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PCV_HIP(hipStreamSynchronize(st));
    });
}

pcv_status pcv_searcher_set_kernel(pcv_searcher* s, int kernel) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "set_kernel: searcher is NULL");
        PCV_REQUIRE(kernel >= PCV_KERNEL_AUTO && kernel <= PCV_KERNEL_MFMA, "set_kernel: unknown kernel %d", kernel);
        std::lock_guard<std::mutex> lk(s->mu);
        s->kernel = kernel;
    });
}

pcv_status pcv_searcher_set_screening_copy(pcv_searcher* s, int mode) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "searcher_set_screening_copy: searcher is NULL");
        refuse_view(s, "set_screening_copy");
        PCV_REQUIRE(mode >= PCV_SCREEN_COPY_OFF && mode <= PCV_SCREEN_COPY_INT8, "searcher_set_screening_copy: unknown mode %d", mode);
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_HIP(hipSetDevice(s->ctx->device));
        if (mode == PCV_SCREEN_COPY_OFF) {
            PCV_HIP(hipStreamSynchronize(s->ctx->stream));
            drop_screening_copies(s);
            s->gen += 1;  // (a view keeps the copies its parent keeps)
        }
        if (mode != PCV_SCREEN_COPY_AUTO && have_six_copies(s)) {  // (the 6-bit copies are AUTO's alone)
            PCV_HIP(hipStreamSynchronize(s->ctx->stream));
            drop_six_copies(s);
            s->gen += 1;
        }
        s->screen_copy = mode;
        s->screen_copy_gave_way = false;
        s->six_gave_way = false;
    });
}

pcv_status pcv_searcher_set_mid_copy(pcv_searcher* s, int mode) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "searcher_set_mid_copy: searcher is NULL");
        refuse_view(s, "set_mid_copy");
        PCV_REQUIRE(mode >= PCV_MID_COPY_OFF && mode <= PCV_MID_COPY_ON, "searcher_set_mid_copy: unknown mode %d", mode);
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "searcher_set_mid_copy: a queued pass has not been collected");
        PCV_HIP(hipSetDevice(s->ctx->device));
        if (mode == PCV_MID_COPY_OFF) {
            PCV_HIP(hipStreamSynchronize(s->ctx->stream));
            drop_mid_copies(s);
        }
        if (mode == PCV_MID_COPY_ON && !s->mids_present) s->dirty = true;  // built by the next finalize
        s->mid_copy = mode;
        s->mid_gave_way = false;
        s->mid_hot_passes = 0;
    });
}

pcv_status pcv_searcher_allow_wide_sharded_pass(pcv_searcher* s, int on) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "allow_wide_sharded_pass: searcher is NULL");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "allow_wide_sharded_pass: a queued pass has not been collected");
        s->wide_sharded = on != 0;
    });
}

pcv_status pcv_searcher_wait_background(pcv_searcher* s) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "wait_background: searcher is NULL");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_HIP(hipSetDevice(s->ctx->device));
        settle_mid_build(s, true);
    });
}

pcv_status pcv_searcher_set_candidate_capacity(pcv_searcher* s, uint32_t n_candidates) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "set_candidate_capacity: searcher is NULL");
        PCV_REQUIRE(n_candidates >= 16 && n_candidates <= (1u << 24), "set_candidate_capacity: %u outside [16, 2^24]", n_candidates);
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "set_candidate_capacity: a queued pass has not been collected");
        PCV_HIP(hipSetDevice(s->ctx->device));
        PCV_HIP(hipStreamSynchronize(s->ctx->stream));
        s->cand_cap = n_candidates;  // the lists are (re)sized to it by the next pass; a pass that needs more grows them
        s->range_cap = 0;
        s->d_cand.release();
        s->d_cand_s.release();
    });
}

pcv_status pcv_searcher_set_tuning(pcv_searcher* s, uint32_t flags) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "set_tuning: searcher is NULL");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "set_tuning: a queued pass has not been collected");
        s->fail_copy_alloc = (flags & (uint32_t)PCV_TUNE_FAIL_COPY_ALLOC) != 0;
        s->scan_flags = flags & ~(uint32_t)PCV_TUNE_FAIL_COPY_ALLOC;
    });
}

pcv_status pcv_searcher_set_shard_offset(pcv_searcher* s, int64_t first_global_pos) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "set_shard_offset: searcher is NULL");
        refuse_view(s, "set_shard_offset");
        std::lock_guard<std::mutex> lk(s->mu);
        s->shard_offset = first_global_pos;
        assign_positions(s);
        s->gen += 1;  // (the parent positions a view's hits carry)
    });
}

pcv_status pcv_searcher_search(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids,
                               int n_sources, int k, int64_t* out_ids, float* out_scores, int* out_counts) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "search: searcher is NULL");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "search: a pass queued by search_device_begin has not been collected");
        sync_view(s);
        std::vector<pcv_hit_dev> hits;
        search_hits(s, queries, n_queries, source_ids, n_sources, k, hits);
        hits_to_outputs(s->metric, s->D, hits.data(), n_queries, k, out_ids, out_scores, out_counts);
    });
}

pcv_status pcv_searcher_search_range(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                     const float* bounds, int64_t max_results, int64_t* out_ids, float* out_scores,
                                     int64_t* out_counts, uint8_t* out_more) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "search_range: searcher is NULL");
        PCV_REQUIRE(queries != nullptr && n_queries > 0, "search_range: no queries");
        PCV_REQUIRE(bounds != nullptr, "search_range: bounds is NULL");
        for (int q = 0; q < n_queries; ++q) PCV_REQUIRE(bounds[q] == bounds[q], "search_range: the bound of query %d is NaN", q);
        PCV_REQUIRE(max_results >= 1 && max_results <= (int64_t)PCV_MAX_RANGE_ROWS, "search_range: max_results %lld outside [1,%d]",
                    (long long)max_results, (int)PCV_MAX_RANGE_ROWS);
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "search_range: a pass queued by search_device_begin has not been collected");
        sync_view(s);
        search_range(s, queries, n_queries, source_ids, n_sources, bounds, max_results, out_ids, out_scores, out_counts, out_more);
    });
}

pcv_status pcv_searcher_search_distinct(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                        int num_results, float threshold, int pool, int64_t* out_ids, float* out_scores,
                                        int32_t* out_counts, int32_t* out_similar, int32_t* out_examined, uint8_t* out_more) {
    return guarded([&] {
        check_ranked_args(s, queries, n_queries, num_results, pool, "search_distinct", (int)PCV_MAX_DISTINCT_POOL);
        PCV_REQUIRE(threshold == threshold, "search_distinct: threshold is NaN");
        PCV_REQUIRE(threshold > -1.0f && threshold <= 1.0f, "search_distinct: threshold %g outside (-1, 1]", (double)threshold);
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "search_distinct: a pass queued by search_device_begin has not been collected");
        sync_view(s);
        search_distinct(RankedCall{s, queries, n_queries, source_ids, n_sources, num_results, pool, out_ids, out_scores, out_counts, out_examined, out_more},
                        threshold, out_similar);
    });
}

pcv_status pcv_searcher_search_diverse(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                       int num_results, float lambda, int pool, int64_t* out_ids, float* out_scores, double* out_marginal,
                                       int32_t* out_ranks, int32_t* out_counts, int32_t* out_examined, uint8_t* out_exact) {
    return guarded([&] {
        check_ranked_args(s, queries, n_queries, num_results, pool, "search_diverse", (int)PCV_MAX_DIVERSE_POOL);
        PCV_REQUIRE(lambda == lambda, "search_diverse: lambda is NaN");
        PCV_REQUIRE(lambda >= 0.0f && lambda <= 1.0f, "search_diverse: lambda %g outside [0, 1]", (double)lambda);
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "search_diverse: a pass queued by search_device_begin has not been collected");
        sync_view(s);
        search_diverse(RankedCall{s, queries, n_queries, source_ids, n_sources, num_results, pool, out_ids, out_scores, out_counts, out_examined, out_exact},
                       lambda, out_marginal, out_ranks);
    });
}

pcv_status pcv_searcher_set_groups(pcv_searcher* s, const int64_t* ids, const int64_t* groups, int64_t n) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "set_groups: searcher is NULL");
        PCV_REQUIRE(n >= 0 && ((ids != nullptr && groups != nullptr) || n == 0), "set_groups: bad lists (NULL with n > 0, or n < 0)");
        for (int64_t i = 0; i < n; ++i)
            PCV_REQUIRE(groups[i] >= PCV_NO_GROUP, "set_groups: group %lld of id %lld (element %lld) is negative and not PCV_NO_GROUP",
                        (long long)groups[i], (long long)ids[i], (long long)i);
        refuse_view(s, "set_groups");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "set_groups: a queued pass has not been collected");
        set_table(s, s->groups, "set_groups", ids, groups, n);
    });
}

pcv_status pcv_searcher_clear_groups(pcv_searcher* s) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "clear_groups: searcher is NULL");
        refuse_view(s, "clear_groups");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "clear_groups: a queued pass has not been collected");
        clear_table(s, s->groups);
    });
}

pcv_status pcv_searcher_get_groups(pcv_searcher* s, const int64_t* ids, int64_t n, int64_t* out_groups) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "get_groups: searcher is NULL");
        PCV_REQUIRE(n >= 0 && ((ids != nullptr && out_groups != nullptr) || n == 0), "get_groups: bad lists (NULL with n > 0, or n < 0)");
        pcv_searcher* owner = s->view_parent ? s->view_parent : s;
        std::lock_guard<std::mutex> lk(owner->mu);
        PCV_REQUIRE(!owner->pending.active, "get_groups: a queued pass has not been collected");
        get_table(owner, owner->groups, ids, n, out_groups);
    });
}

pcv_status pcv_searcher_group_stats(pcv_searcher* s, pcv_group_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "group_stats: NULL argument");
        pcv_searcher* owner = s->view_parent ? s->view_parent : s;
        std::lock_guard<std::mutex> lk(owner->mu);
        const pcv_searcher::IdTable& t = owner->groups;
        *out = pcv_group_stats{t.head.ids, t.head.entries, (int64_t)t.slots, t.rehashes, t.last_set_ms};
    });
}

pcv_status pcv_searcher_search_grouped(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                       int num_results, int pool, int64_t* out_ids, float* out_scores, int64_t* out_groups,
                                       int32_t* out_counts, int32_t* out_collapsed, int32_t* out_examined, uint8_t* out_more) {
    return guarded([&] {
        check_ranked_args(s, queries, n_queries, num_results, pool, "search_grouped", (int)PCV_MAX_GROUPED_POOL);
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "search_grouped: a pass queued by search_device_begin has not been collected");
        sync_view(s);
        // (a view reads its parent's table: the parent stays locked while the kernels may follow its pointers)
        std::unique_lock<std::mutex> plk;
        if (s->view_parent) plk = std::unique_lock<std::mutex>(s->view_parent->mu);
        search_grouped(RankedCall{s, queries, n_queries, source_ids, n_sources, num_results, pool, out_ids, out_scores, out_counts, out_examined, out_more},
                       s->view_parent ? s->view_parent : s, out_groups, out_collapsed);
    });
}

pcv_status pcv_searcher_set_values(pcv_searcher* s, const int64_t* ids, const int64_t* values, int64_t n) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "set_values: searcher is NULL");
        PCV_REQUIRE(n >= 0 && ((ids != nullptr && values != nullptr) || n == 0), "set_values: bad lists (NULL with n > 0, or n < 0)");
        refuse_view(s, "set_values");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "set_values: a queued pass has not been collected");
        if (n == 0) return;
        const auto bump = at_exit([&] { s->values_gen += 1; });  // (also when the call fails half way: the table may have changed)
        set_table(s, s->values, "set_values", ids, values, n);
    });
}

pcv_status pcv_searcher_clear_values(pcv_searcher* s) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "clear_values: searcher is NULL");
        refuse_view(s, "clear_values");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "clear_values: a queued pass has not been collected");
        const auto bump = at_exit([&] { s->values_gen += 1; });
        clear_table(s, s->values);
    });
}

pcv_status pcv_searcher_get_values(pcv_searcher* s, const int64_t* ids, int64_t n, int64_t* out_values) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "get_values: searcher is NULL");
        PCV_REQUIRE(n >= 0 && ((ids != nullptr && out_values != nullptr) || n == 0), "get_values: bad lists (NULL with n > 0, or n < 0)");
        pcv_searcher* owner = s->view_parent ? s->view_parent : s;
        std::lock_guard<std::mutex> lk(owner->mu);
        PCV_REQUIRE(!owner->pending.active, "get_values: a queued pass has not been collected");
        get_table(owner, owner->values, ids, n, out_values);
    });
}

pcv_status pcv_searcher_value_stats(pcv_searcher* s, pcv_value_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "value_stats: NULL argument");
        pcv_searcher* owner = s->view_parent ? s->view_parent : s;
        std::lock_guard<std::mutex> lk(owner->mu);
        const pcv_searcher::IdTable& t = owner->values;
        *out = pcv_value_stats{t.head.ids, t.head.entries, (int64_t)t.slots, t.rehashes, t.last_set_ms};
    });
}

pcv_status pcv_searcher_count_where(pcv_searcher* s, const int64_t* source_ids, int n_sources, int64_t lo, int64_t hi, uint32_t flags,
                                    int64_t* out_rows, int64_t* out_searchable) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "count_where: searcher is NULL");
        PCV_REQUIRE(n_sources >= 0 && (source_ids != nullptr || n_sources == 0), "count_where: bad source list (NULL with n_sources > 0, or n_sources < 0)");
        const WherePred w = check_where(lo, hi, flags, "count_where");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "count_where: a queued pass has not been collected");
        sync_view(s);
        std::unique_lock<std::mutex> plk;  // (as in search_grouped: the parent's table is read)
        if (s->view_parent) plk = std::unique_lock<std::mutex>(s->view_parent->mu);
        count_where(s, s->view_parent ? s->view_parent : s, source_ids, n_sources, w, out_rows, out_searchable);
    });
}

pcv_status pcv_searcher_search_where(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                     int num_results, int pool, int64_t lo, int64_t hi, uint32_t flags, int64_t* out_ids, float* out_scores,
                                     int64_t* out_values, int32_t* out_counts, int32_t* out_examined, uint8_t* out_more) {
    return guarded([&] {
        check_ranked_args(s, queries, n_queries, num_results, pool, "search_where", (int)PCV_MAX_WHERE_POOL);
        const WherePred w = check_where(lo, hi, flags, "search_where");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "search_where: a pass queued by search_device_begin has not been collected");
        sync_view(s);
        // (a view reads its parent's table: the parent stays locked while the kernels may follow its pointers)
        std::unique_lock<std::mutex> plk;
        if (s->view_parent) plk = std::unique_lock<std::mutex>(s->view_parent->mu);
        search_where(RankedCall{s, queries, n_queries, source_ids, n_sources, num_results, pool, out_ids, out_scores, out_counts, out_examined, out_more},
                     s->view_parent ? s->view_parent : s, w, out_values);
    });
}

pcv_status pcv_searcher_search_boosted(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                       int num_results, int pool, const pcv_boost* boost, int64_t* out_ids, float* out_scores,
                                       double* out_boosted, int64_t* out_values, int32_t* out_ranks, int32_t* out_counts,
                                       int32_t* out_examined, uint8_t* out_exact) {
    return guarded([&] {
        check_ranked_args(s, queries, n_queries, num_results, pool, "search_boosted", (int)PCV_MAX_BOOST_POOL);
        PCV_REQUIRE(boost != nullptr, "search_boosted: boost is NULL");
        PCV_REQUIRE(boost->n_knots >= 1 && boost->n_knots <= (int)PCV_MAX_BOOST_KNOTS, "search_boosted: n_knots %d outside [1,%d]", boost->n_knots,
                    (int)PCV_MAX_BOOST_KNOTS);
        pcv_boost b{};  // (the knots in use and nothing else: what lies behind them never reaches the device)
        b.n_knots = boost->n_knots;
        b.unset_boost = boost->unset_boost;
        PCV_REQUIRE(std::isfinite(b.unset_boost), "search_boosted: unset_boost is not finite");
        for (int j = 0; j < b.n_knots; ++j) {
            b.knot_values[j] = boost->knot_values[j];
            b.knot_boosts[j] = boost->knot_boosts[j];
            PCV_REQUIRE(b.knot_values[j] != PCV_NO_VALUE, "search_boosted: knot value %d is PCV_NO_VALUE", j);
            PCV_REQUIRE(j == 0 || b.knot_values[j] > b.knot_values[j - 1], "search_boosted: knot values are not strictly increasing (knot %d)", j);
            PCV_REQUIRE(std::isfinite(b.knot_boosts[j]), "search_boosted: knot boost %d is not finite", j);
        }
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "search_boosted: a pass queued by search_device_begin has not been collected");
        sync_view(s);
        // (a view reads its parent's table: the parent stays locked while the kernels may follow its pointers)
        std::unique_lock<std::mutex> plk;
        if (s->view_parent) plk = std::unique_lock<std::mutex>(s->view_parent->mu);
        search_boosted(RankedCall{s, queries, n_queries, source_ids, n_sources, num_results, pool, out_ids, out_scores, out_counts, out_examined, out_exact},
                       s->view_parent ? s->view_parent : s, b, out_boosted, out_values, out_ranks);
    });
}

// What both compound calls ask of their scalar arguments and of the two levels of offsets, before anything touches the searcher.
static void check_compound_args(const pcv_searcher* s, int n_compounds, int num_results, int pool, int mode, float avoid_weight, const char* who) {
    PCV_REQUIRE(s != nullptr, "%s: searcher is NULL", who);
    PCV_REQUIRE(n_compounds > 0 && n_compounds <= (1 << 20), "%s: n_compounds %d outside [1,%d]", who, n_compounds, 1 << 20);
    PCV_REQUIRE(num_results >= 1 && num_results <= (int)PCV_MAX_RESULTS, "%s: num_results %d outside [1,%d]", who, num_results,
                (int)PCV_MAX_RESULTS);
    PCV_REQUIRE(pool >= num_results && pool <= (int)PCV_MAX_COMPOUND_POOL, "%s: pool %d outside [num_results = %d, %d]", who, pool, num_results,
                (int)PCV_MAX_COMPOUND_POOL);
    PCV_REQUIRE(mode == PCV_COMPOUND_ALL || mode == PCV_COMPOUND_ANY, "%s: unknown mode %d", who, mode);
    PCV_REQUIRE(std::isfinite(avoid_weight) && avoid_weight >= 0.0f, "%s: avoid_weight %g is negative or not finite", who, (double)avoid_weight);
}
// offsets[n + 1] of one side: from 0, ascending, every compound with lo .. PCV_MAX_COMPOUND_PARTS vectors
static void check_compound_offsets(const int64_t* off, int n, int lo, const char* side, const char* who) {
    PCV_REQUIRE(off != nullptr, "%s: %s_offsets is NULL", who, side);
    PCV_REQUIRE(off[0] == 0, "%s: %s_offsets[0] must be 0", who, side);
    for (int i = 0; i < n; ++i) {
        PCV_REQUIRE(off[i + 1] >= off[i], "%s: %s_offsets are not ascending (%s_offsets[%d] < %s_offsets[%d])", who, side, side, i + 1, side, i);
        const int64_t w = off[i + 1] - off[i];
        PCV_REQUIRE(w >= lo && w <= (int64_t)PCV_MAX_COMPOUND_PARTS, "%s: compound %d has %lld %s vectors, outside [%d,%d]", who, i, (long long)w,
                    side, lo, (int)PCV_MAX_COMPOUND_PARTS);
    }
}
// n vectors of one side: every value finite and, under the cosine, a squared norm finish_score accepts
static void check_compound_vectors(const pcv_searcher* s, const float* v, int64_t n, const char* side, const char* who) {
    for (int64_t q = 0; q < n; ++q) {
        const float* x = v + (size_t)q * s->D;
        for (int i = 0; i < s->D; ++i)
            PCV_REQUIRE(std::isfinite(x[i]), "%s: value %d of %s vector %lld is not finite", who, i, side, (long long)q);
        if (s->metric != PCV_METRIC_COSINE) continue;
        const double nq = query_norm2(x, s->D);
        PCV_REQUIRE(nq >= 0x1p-126 && nq < (double)INFINITY, "%s: %s vector %lld has squared norm %g: no cosine is defined for it", who, side,
                    (long long)q, nq);
    }
}

pcv_status pcv_searcher_search_compound(pcv_searcher* s, const int64_t* source_ids, int n_sources, int num_results, int pool, int mode,
                                        float avoid_weight, const float* want, const int64_t* want_offsets, const float* avoid,
                                        const int64_t* avoid_offsets, int n_compounds, int64_t* out_ids, double* out_combined,
                                        float* out_part_scores, double* out_penalties, int32_t* out_counts, int32_t* out_examined,
                                        uint8_t* out_exact) {
    return guarded([&] {
        const char* who = "search_compound";
        check_compound_args(s, n_compounds, num_results, pool, mode, avoid_weight, who);
        check_compound_offsets(want_offsets, n_compounds, 1, "want", who);
        PCV_REQUIRE(want != nullptr, "%s: want is NULL", who);
        PCV_REQUIRE(avoid == nullptr || avoid_offsets != nullptr, "%s: avoid is given without avoid_offsets", who);
        if (avoid_offsets) {
            check_compound_offsets(avoid_offsets, n_compounds, 0, "avoid", who);
            PCV_REQUIRE(avoid != nullptr || avoid_offsets[n_compounds] == 0, "%s: avoid is NULL with %lld avoided vectors", who,
                        (long long)avoid_offsets[n_compounds]);
        }
        std::lock_guard<std::mutex> lk(s->mu);
        check_compound_vectors(s, want, want_offsets[n_compounds], "wanted", who);
        if (avoid_offsets) check_compound_vectors(s, avoid, avoid_offsets[n_compounds], "avoided", who);
        PCV_REQUIRE(!s->pending.active, "%s: a pass queued by search_device_begin has not been collected", who);
        sync_view(s);
        search_compound(CompoundCall{s, source_ids, n_sources, num_results, pool, mode, (double)avoid_weight, want, want_offsets, avoid, avoid_offsets,
                                     n_compounds, out_ids, out_combined, out_part_scores, out_penalties, out_counts, out_examined, out_exact});
    });
}

pcv_status pcv_searcher_search_compound_like(pcv_searcher* s, const int64_t* source_ids, int n_sources, int num_results, int pool, int mode,
                                             float avoid_weight, const int64_t* want_ids, const float* want_weights,
                                             const int64_t* want_example_offsets, const int64_t* want_offsets, const int64_t* avoid_ids,
                                             const float* avoid_weights, const int64_t* avoid_example_offsets,
                                             const int64_t* avoid_offsets, int n_compounds, int exclude_examples, int64_t* out_ids,
                                             double* out_combined, float* out_part_scores, double* out_penalties, int32_t* out_counts,
                                             int32_t* out_examined, uint8_t* out_exact) {
    return guarded([&] {
        const char* who = "search_compound_like";
        check_compound_args(s, n_compounds, num_results, pool, mode, avoid_weight, who);
        check_compound_offsets(want_offsets, n_compounds, 1, "want", who);
        const int n_want = (int)want_offsets[n_compounds];
        check_like_args(s, want_ids, want_weights, want_example_offsets, n_want, who);
        const bool avoiding = avoid_offsets != nullptr;
        PCV_REQUIRE(avoiding == (avoid_example_offsets != nullptr) && (avoiding || (avoid_ids == nullptr && avoid_weights == nullptr)),
                    "%s: the avoided side must be given whole (offsets at both levels) or left NULL", who);
        int n_avoid = 0;
        if (avoiding) {
            check_compound_offsets(avoid_offsets, n_compounds, 0, "avoid", who);
            n_avoid = (int)avoid_offsets[n_compounds];
            check_like_args(s, avoid_ids, avoid_weights, avoid_example_offsets, n_avoid, who);
        }
        std::lock_guard<std::mutex> lk(s->mu);
        sync_view(s);
        LikeBuilt wanted, avoided;
        {
            pcv_searcher* owner = nullptr;
            const auto owner_lock = lock_like_owner(s, owner, who);
            build_like_queries(owner, want_ids, want_weights, want_example_offsets, n_want, true, nullptr, wanted);
            if (avoiding) build_like_queries(owner, avoid_ids, avoid_weights, avoid_example_offsets, n_avoid, true, nullptr, avoided);
        }
        check_compound_vectors(s, wanted.vectors.data(), n_want, "wanted", who);
        if (avoiding) check_compound_vectors(s, avoided.vectors.data(), n_avoid, "avoided", who);
        CompoundCall call{s, source_ids, n_sources, num_results, pool, mode, (double)avoid_weight, wanted.vectors.data(), want_offsets,
                          avoiding ? avoided.vectors.data() : nullptr, avoid_offsets, n_compounds, out_ids, out_combined, out_part_scores,
                          out_penalties, out_counts, out_examined, out_exact};
        // Exclusion: at most `spare` rows carry a wanted example id of any one compound, so the first num_results + spare rows of its
        // answer hold the num_results best of the others; what certifies the longer answer certifies its head.
        int64_t spare = 0;
        if (exclude_examples)
            for (int i = 0; i < n_compounds; ++i) {
                int64_t n = 0;
                for (int64_t p = want_offsets[i]; p < want_offsets[i + 1]; ++p) n += wanted.carrier_rows[(size_t)p];
                spare = std::max(spare, n);
            }
        if (spare == 0) {
            search_compound(call);
            return;
        }
        if ((int64_t)num_results + spare > (int64_t)PCV_MAX_RESULTS)
            PCV_FAIL(PCV_ERR_UNSUPPORTED, "%s: num_results %d plus %lld example rows to leave out is more than %d", who, num_results,
                     (long long)spare, (int)PCV_MAX_RESULTS);
        const int k = num_results, kk = num_results + (int)spare, P = (int)PCV_MAX_COMPOUND_PARTS;
        const size_t n = (size_t)n_compounds * kk;
        std::vector<int64_t> ids(n);
        std::vector<double> combined(n), penalties(n);
        std::vector<float> parts(n * P);
        std::vector<int32_t> counts((size_t)n_compounds);
        call.k = kk;
        call.pool = std::max(pool, kk);
        call.out_ids = ids.data(), call.out_combined = combined.data(), call.out_part_scores = parts.data(), call.out_penalties = penalties.data();
        call.out_counts = counts.data();
        search_compound(call);
        std::vector<int64_t> own;
        for (int i = 0; i < n_compounds; ++i) {
            own.assign(want_ids + want_example_offsets[want_offsets[i]], want_ids + want_example_offsets[want_offsets[i + 1]]);
            std::sort(own.begin(), own.end());
            int at = 0;
            for (int j = 0; j < kk; ++j) {
                const size_t from = (size_t)i * kk + j, to = (size_t)i * k + at;
                const bool take = j < counts[(size_t)i] && at < k && !std::binary_search(own.begin(), own.end(), ids[from]);
                if (!take) continue;
                if (out_ids) out_ids[to] = ids[from];
                if (out_combined) out_combined[to] = combined[from];
                if (out_penalties) out_penalties[to] = penalties[from];
                if (out_part_scores) std::memcpy(out_part_scores + to * P, parts.data() + from * P, (size_t)P * sizeof(float));
                ++at;
            }
            if (out_counts) out_counts[i] = at;
            for (; at < k; ++at) {
                const size_t to = (size_t)i * k + at;
                if (out_ids) out_ids[to] = -1;
                if (out_combined) out_combined[to] = NAN;
                if (out_penalties) out_penalties[to] = NAN;
                if (out_part_scores)
                    for (int u = 0; u < P; ++u) out_part_scores[to * P + u] = NAN;
            }
        }
    });
}

pcv_status pcv_searcher_last_select_stats(pcv_searcher* s, float* out_ms, int32_t* out_launches) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "last_select_stats: searcher is NULL");
        std::lock_guard<std::mutex> lk(s->mu);
        if (out_ms) *out_ms = s->select_ms;
        if (out_launches) *out_launches = s->select_launches;
    });
}

pcv_status pcv_searcher_like_queries(pcv_searcher* s, const int64_t* example_ids, const float* weights, const int64_t* offsets,
                                     int n_queries, float* out_queries, void* d_out_queries, uint8_t* out_found,
                                     int64_t* out_member_rows) {
    return guarded([&] {
        const int64_t n = check_like_args(s, example_ids, weights, offsets, n_queries, "like_queries");
        std::lock_guard<std::mutex> lk(s->mu);
        sync_view(s);
        pcv_searcher* owner = nullptr;
        const auto owner_lock = lock_like_owner(s, owner, "like_queries");
        LikeBuilt built;
        build_like_queries(owner, example_ids, weights, offsets, n_queries, out_queries != nullptr, d_out_queries, built);
        if (out_queries && n_queries > 0) std::memcpy(out_queries, built.vectors.data(), built.vectors.size() * sizeof(float));
        if (out_found && n > 0) std::memcpy(out_found, built.found.data(), (size_t)n);
        if (out_member_rows && n_queries > 0) std::memcpy(out_member_rows, built.member_rows.data(), (size_t)n_queries * sizeof(int64_t));
    });
}

pcv_status pcv_searcher_search_like(pcv_searcher* s, const int64_t* example_ids, const float* weights, const int64_t* offsets,
                                    int n_queries, const int64_t* source_ids, int n_sources, int k, int exclude_examples,
                                    int64_t* out_ids, float* out_scores, int* out_counts, uint8_t* out_found) {
    return guarded([&] {
        const int64_t n = check_like_args(s, example_ids, weights, offsets, n_queries, "search_like");
        PCV_REQUIRE(k > 0 && k <= (1 << 24), "search_like: num_results %d outside [1,%d]", k, 1 << 24);
        std::lock_guard<std::mutex> lk(s->mu);
        sync_view(s);
        LikeBuilt built;
        {
            pcv_searcher* owner = nullptr;
            const auto owner_lock = lock_like_owner(s, owner, "search_like");
            build_like_queries(owner, example_ids, weights, offsets, n_queries, true, nullptr, built);
        }
        if (out_found && n > 0) std::memcpy(out_found, built.found.data(), (size_t)n);
        if (n_queries == 0) return;
        // Exclusion: at most carrier_rows[q] rows carry one of q's example ids, so the first k + max_q carrier_rows[q] hits hold
        // the k best of the others — exact whatever the surplus, since num_results is not limited.
        int64_t spare = 0;
        bool any = false;
        for (int q = 0; q < n_queries; ++q) {
            any = any || built.member_rows[(size_t)q] > 0;
            if (exclude_examples) spare = std::max(spare, built.carrier_rows[(size_t)q]);
        }
        PCV_REQUIRE((int64_t)k + spare <= (1 << 24), "search_like: num_results %d plus %lld example rows to leave out is more than %d", k,
                    (long long)spare, 1 << 24);
        const int kk = k + (int)spare;
        const pcv_hit_dev none{NAN, -1, -1};
        std::vector<pcv_hit_dev> hits;
        if (any)
            search_hits(s, built.vectors.data(), n_queries, source_ids, n_sources, kk, hits);
        else {  // no query has a member: nothing to search for
            PCV_REQUIRE(!s->dirty, "search_like: rows were added or cleared without pcv_searcher_finalize");
            hits.assign((size_t)n_queries * kk, none);
            s->stats = pcv_scan_stats{};
        }
        std::vector<pcv_hit_dev> kept((size_t)n_queries * k, none);
        std::vector<int64_t> own;
        for (int q = 0; q < n_queries; ++q) {
            if (built.member_rows[(size_t)q] == 0) continue;  // a query without members has no results
            own.clear();
            if (exclude_examples) {
                own.assign(example_ids + offsets[q], example_ids + offsets[q + 1]);
                std::sort(own.begin(), own.end());
            }
            int at = 0;
            for (int j = 0; j < kk && at < k; ++j) {
                const pcv_hit_dev& h = hits[(size_t)q * kk + j];
                if (h.pos < 0) continue;
                if (exclude_examples && std::binary_search(own.begin(), own.end(), h.id)) continue;
                kept[(size_t)q * k + at++] = h;
            }
        }
        hits_to_outputs(s->metric, s->D, kept.data(), n_queries, k, out_ids, out_scores, out_counts);
    });
}

pcv_status pcv_searcher_search_device(pcv_searcher* s, const float* queries, int n_queries,
                                      const int64_t* source_ids, int n_sources, int k, void* d_out, int async) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && d_out != nullptr, "search_device: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        check_search_args(s, queries, n_queries, k, "search_device");
        PCV_REQUIRE(!s->pending.active, "search_device: a pass queued by search_device_begin has not been collected");
        sync_view(s);
        const SearchPlan plan = plan_search(s, source_ids, n_sources, n_queries);
        const int qstep = plan.qstep;
        pcv_hit_dev* out = (pcv_hit_dev*)d_out;
        if (!open_search(s, plan)) {
            const pcv_hit_dev none{NAN, -1, -1};
            std::vector<pcv_hit_dev> hits((size_t)n_queries * k, none);
            PCV_HIP(hipMemcpyAsync(out, hits.data(), hits.size() * sizeof(pcv_hit_dev), hipMemcpyHostToDevice, s->ctx->stream));
            PCV_HIP(hipStreamSynchronize(s->ctx->stream));  // `hits` dies with this scope
            return;
        }
        // results stay on the device: every pass writes its slice of the caller's list
        for (int q0 = 0; q0 < n_queries; q0 += qstep) {
            const int B = std::min(qstep, n_queries - q0);
            run_pass(s, PassRequest(queries + (size_t)q0 * s->D, B, plan.segs, plan.kernel).top_k(k, out + (size_t)q0 * k, false));
            if (s->view_parent) launch_view_remap(s->ctx->stream, out + (size_t)q0 * k, (int64_t)B * k, s->d_ppos.p, s->view_rows);
        }
        if (s->view_parent) PCV_HIP(hipStreamSynchronize(s->ctx->stream));
        (void)async;  // every pass has been collected: nothing is left in flight
    });
}

pcv_status pcv_searcher_search_device_begin(pcv_searcher* s, const float* queries, int n_queries,
                                            const int64_t* source_ids, int n_sources, int k, void* d_out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && d_out != nullptr, "search_device_begin: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        device_begin(s, queries, n_queries, source_ids, n_sources, k, (pcv_hit_dev*)d_out);
    });
}

pcv_status pcv_searcher_search_device_begin_dq(pcv_searcher* s, const void* d_queries, int n_queries,
                                               const int64_t* source_ids, int n_sources, int k, void* d_out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && d_out != nullptr, "search_device_begin_dq: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        device_begin(s, (const float*)d_queries, n_queries, source_ids, n_sources, k, (pcv_hit_dev*)d_out, true);
    });
}

pcv_status pcv_searcher_search_device_end(pcv_searcher* s, int* out_overflowed) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "search_device_end: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_HIP(hipSetDevice(s->ctx->device));
        const bool over = finish_pass(s);
        if (out_overflowed) *out_overflowed = over ? 1 : 0;
    });
}

pcv_status pcv_searcher_repeat_without_guess(pcv_searcher* s) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "repeat_without_guess: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        s->spec_hold = true;  // cleared by the next pass that completes (finish_pass)
    });
}

static pcv_status similarity(pcv_ctx* ctx, const float* a, int B, const float* m, int64_t N, int dim, float* out,
                             int cosine) {
    return guarded([&] {
        PCV_REQUIRE(ctx != nullptr && a != nullptr && m != nullptr && out != nullptr, "similarity: NULL argument");
        PCV_REQUIRE(B > 0 && N > 0 && dim > 0, "similarity: empty input");
        PCV_HIP(hipSetDevice(ctx->device));
        DevBuf<float> d_a, d_m, d_o;
        d_a.ensure((size_t)B * dim);
        d_m.ensure((size_t)N * dim);
        d_o.ensure((size_t)B * N);
        PCV_HIP(hipMemcpyAsync(d_a.p, a, (size_t)B * dim * 4, hipMemcpyHostToDevice, ctx->stream));
        PCV_HIP(hipMemcpyAsync(d_m.p, m, (size_t)N * dim * 4, hipMemcpyHostToDevice, ctx->stream));
        launch_similarity_matrix(ctx->stream, d_a.p, B, d_m.p, N, dim, cosine, d_o.p);
        PCV_HIP(hipMemcpyAsync(out, d_o.p, (size_t)B * N * 4, hipMemcpyDeviceToHost, ctx->stream));
        PCV_HIP(hipStreamSynchronize(ctx->stream));
        PCV_HIP(hipGetLastError());
    });
}

pcv_status pcv_dot_product(pcv_ctx* ctx, const float* a, int B, const float* m, int64_t N, int dim, float* out) {
    return similarity(ctx, a, B, m, N, dim, out, 0);
}
pcv_status pcv_cosine_similarity(pcv_ctx* ctx, const float* a, int B, const float* m, int64_t N, int dim,
                                 float* out) {
    return similarity(ctx, a, B, m, N, dim, out, 1);
}

pcv_status pcv_searcher_last_stats(pcv_searcher* s, pcv_scan_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->stats;
    });
}

}  // extern "C"
