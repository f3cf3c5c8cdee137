// searcher_exchange.cpp — searching across shards: the merge of per-shard lists (pcv_merge_topk*), the RCCL communicator
// (pcv_comm_*) and the sharded search built on the begin / end pass of searcher_calls.cpp.  C entry points only: each takes the
// lock of the searcher it is given; a communicator is used by one thread at a time.
#include <dlfcn.h>

#include <cstring>
#include <string>

#include "searcher_calls.h"

using namespace pcv;

extern "C" {

namespace {
// merge scratch of a context: device output and its pinned host copy for `n` records
void ensure_merge_scratch(pcv_ctx* ctx, size_t n) {
    if (ctx->merge_cap >= n) return;
    PCV_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->merge_dev) (void)hipFree(ctx->merge_dev);
    if (ctx->merge_pin) (void)hipHostFree(ctx->merge_pin);
    ctx->merge_dev = ctx->merge_pin = nullptr;
    ctx->merge_cap = 0;
    PCV_HIP(hipMalloc(&ctx->merge_dev, n * sizeof(pcv_hit_dev)));
    PCV_HIP(hipHostMalloc(&ctx->merge_pin, n * sizeof(pcv_hit_dev), hipHostMallocDefault));
    ctx->merge_cap = n;
}

void merge_lists(pcv_ctx* ctx, int metric, int dim, const void* d_lists, int n_shards, int n_queries, int k,
                 int64_t* out_ids, float* out_scores, int* out_counts, int* out_any_overflow) {
    PCV_REQUIRE(ctx != nullptr && d_lists != nullptr, "merge_topk: NULL argument");
    PCV_REQUIRE(n_shards > 0 && n_queries > 0 && k > 0 && k <= kMaxK, "merge_topk: bad shape");
    PCV_HIP(hipSetDevice(ctx->device));
    const int flagged = out_any_overflow != nullptr;
    const size_t n = (size_t)n_queries * k;
    ensure_merge_scratch(ctx, n + 1);
    pcv_hit_dev* d_out = (pcv_hit_dev*)ctx->merge_dev;
    pcv_hit_dev* h_out = (pcv_hit_dev*)ctx->merge_pin;
    launch_merge(ctx->stream, (const pcv_hit_dev*)d_lists, n_shards, n_queries, k, d_out, flagged);
    PCV_HIP(hipMemcpyAsync(h_out, d_out, (n + flagged) * sizeof(pcv_hit_dev), hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP(hipStreamSynchronize(ctx->stream));
    PCV_HIP(hipGetLastError());
    if (flagged) *out_any_overflow = h_out[n].pos != 0;
    hits_to_outputs(metric, dim, h_out, n_queries, k, out_ids, out_scores, out_counts);
}
}  // namespace

pcv_status pcv_merge_topk(pcv_ctx* ctx, int metric, int dim, const void* d_lists, int n_shards, int n_queries,
                          int k, int64_t* out_ids, float* out_scores, int* out_counts) {
    return guarded([&] {
        merge_lists(ctx, metric, dim, d_lists, n_shards, n_queries, k, out_ids, out_scores, out_counts, nullptr);
    });
}

pcv_status pcv_merge_topk_flagged(pcv_ctx* ctx, int metric, int dim, const void* d_lists, int n_shards,
                                  int n_queries, int k, int64_t* out_ids, float* out_scores, int* out_counts,
                                  int* out_any_overflow) {
    return guarded([&] {
        PCV_REQUIRE(out_any_overflow != nullptr, "merge_topk_flagged: NULL argument");
        merge_lists(ctx, metric, dim, d_lists, n_shards, n_queries, k, out_ids, out_scores, out_counts,
                    out_any_overflow);
    });
}

pcv_status pcv_merge_topk_host(int metric, int dim, const pcv_hit* lists, int n_shards, int n_queries, int k,
                               int64_t* out_ids, float* out_scores, int* out_counts) {
    return guarded([&] {
        PCV_REQUIRE(lists != nullptr, "merge_topk_host: lists is NULL");
        PCV_REQUIRE(n_shards > 0 && n_queries > 0 && k > 0 && k <= kMaxK, "merge_topk_host: bad shape");
        static_assert(sizeof(pcv_hit) == sizeof(pcv_hit_dev), "hit layout");
        const pcv_hit_dev* L = reinterpret_cast<const pcv_hit_dev*>(lists);
        const pcv_hit_dev none{NAN, -1, -1};
        std::vector<pcv_hit_dev> out((size_t)n_queries * k, none), m;
        for (int q = 0; q < n_queries; ++q) {
            m.clear();
            for (int r = 0; r < n_shards; ++r)
                for (int j = 0; j < k; ++j) {
                    const pcv_hit_dev& e = L[((size_t)r * n_queries + q) * k + j];
                    if (e.pos >= 0 && e.score == e.score) m.push_back(e);
                }
            std::sort(m.begin(), m.end(), hit_better);  // search.rs:179, canonical order
            for (int j = 0; j < k && j < (int)m.size(); ++j) out[(size_t)q * k + j] = m[j];  // search.rs:180
        }
        hits_to_outputs(metric, dim, out.data(), n_queries, k, out_ids, out_scores, out_counts);
    });
}

// ---- native RCCL exchange ------------------------------------------------------------------------
extern "C++" {
struct NcclId {  // ncclUniqueId of rccl.h: 128 opaque bytes, passed by value
    char internal[128];
};
namespace {
// the handful of RCCL entry points used, resolved from librccl.so.1 at first use (rccl.h signatures)
struct Rccl {
    int (*GetUniqueId)(void* id) = nullptr;
    int (*CommInitRank)(void** comm, int nranks, NcclId id, int rank) = nullptr;
    int (*AllGather)(const void* send, void* recv, size_t count, int dtype, void* comm, hipStream_t st) = nullptr;
    int (*CommDestroy)(void* comm) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false;
};
Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;  // first use may come from two contexts' threads at once
    std::call_once(once, [] {
        // RCCL must sit on the HIP runtime this library is bound to.  A process may hold a second
        // runtime + RCCL pair (PyTorch bundles its own, with the same sonames), so RCCL is looked up by
        // path next to our libamdhip64 first and by soname only after that.
        void* h = nullptr;
        Dl_info info;
        if (dladdr((void*)&hipGetDeviceCount, &info) && info.dli_fname) {
            std::string dir(info.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) {
                dir.resize(slash + 1);
                for (const char* name : {"librccl.so.1", "librccl.so"})
                    if (!h) h = dlopen((dir + name).c_str(), RTLD_NOW | RTLD_LOCAL);
            }
        }
        for (const char* name : {"librccl.so.1", "librccl.so"})
            if (!h) h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (h) {
            r.GetUniqueId = (int (*)(void*))dlsym(h, "ncclGetUniqueId");
            r.CommInitRank = (int (*)(void**, int, NcclId, int))dlsym(h, "ncclCommInitRank");
            r.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
            r.CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
            r.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
            r.ok = r.GetUniqueId && r.CommInitRank && r.AllGather && r.CommDestroy;
        }
    });
    return r;
}
void rccl_check(int rc, const char* what) {
    if (rc != 0) {
        Rccl& r = rccl();
        PCV_FAIL(PCV_ERR_DEVICE, "%s failed: %s", what, r.GetErrorString ? r.GetErrorString(rc) : "RCCL error");
    }
}
}  // namespace

struct pcv_comm {
    pcv_ctx* ctx = nullptr;
    void* comm = nullptr;
    int world = 1, rank = 0;
    DevBuf<pcv_hit_dev> d_local, d_gathered, d_merged;
    PinBuf<pcv_hit_dev> pin_hits;
};
}  // extern "C++"

pcv_status pcv_comm_unique_id(uint8_t out_id[128]) {
    return guarded([&] {
        PCV_REQUIRE(out_id != nullptr, "comm_unique_id: NULL argument");
        if (!rccl().ok) PCV_FAIL(PCV_ERR_UNSUPPORTED, "RCCL (librccl.so.1) is not available: %s", dlerror() ? dlerror() : "");
        NcclId id;
        rccl_check(rccl().GetUniqueId(&id), "ncclGetUniqueId");
        std::memcpy(out_id, id.internal, 128);
    });
}

pcv_status pcv_comm_create(pcv_ctx* ctx, int world_size, int rank, const uint8_t id_bytes[128], pcv_comm** out) {
    return guarded([&] {
        PCV_REQUIRE(ctx != nullptr && id_bytes != nullptr && out != nullptr, "comm_create: NULL argument");
        *out = nullptr;
        PCV_REQUIRE(world_size >= 1 && rank >= 0 && rank < world_size, "comm_create: rank %d / world %d", rank, world_size);
        if (!rccl().ok) PCV_FAIL(PCV_ERR_UNSUPPORTED, "RCCL (librccl.so.1) is not available");
        PCV_HIP(hipSetDevice(ctx->device));
        auto c = std::make_unique<pcv_comm>();
        c->ctx = ctx;
        c->world = world_size;
        c->rank = rank;
        NcclId id;
        std::memcpy(id.internal, id_bytes, 128);
        rccl_check(rccl().CommInitRank(&c->comm, world_size, id, rank), "ncclCommInitRank");
        *out = c.release();
    });
}

pcv_status pcv_comm_destroy(pcv_comm* c) {
    return guarded([&] {
        if (!c) return;
        (void)hipSetDevice(c->ctx->device);
        (void)hipStreamSynchronize(c->ctx->stream);
        if (c->comm) rccl().CommDestroy(c->comm);
        c->d_local.release();
        c->d_gathered.release();
        c->d_merged.release();
        delete c;
    });
}

pcv_status pcv_comm_all_gather(pcv_comm* c, const void* d_send, void* d_recv, size_t bytes_per_rank) {
    return guarded([&] {
        PCV_REQUIRE(c != nullptr && d_send != nullptr && d_recv != nullptr && bytes_per_rank > 0, "comm_all_gather: bad argument");
        PCV_HIP(hipSetDevice(c->ctx->device));
        rccl_check(rccl().AllGather(d_send, d_recv, bytes_per_rank, /*ncclInt8*/ 0, c->comm, c->ctx->stream), "ncclAllGather");
    });
}

static pcv_status search_sharded_impl(pcv_searcher* s, pcv_comm* c, const float* queries, bool queries_on_device, int n_queries,
                                      const int64_t* source_ids, int n_sources, int k, int64_t* out_ids,
                                      float* out_scores, int* out_counts) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && c != nullptr, "search_sharded: NULL argument");
        PCV_REQUIRE(s->ctx == c->ctx, "search_sharded: searcher and communicator live on different contexts");
        // the whole step — local pass, exchange, merge, collection — is one critical section of the searcher:
        // it shares the pass workspace, the pinned blocks and the stream with plain searches
        std::lock_guard<std::mutex> lk(s->mu);
        check_search_args(s, queries, n_queries, k, "search_sharded", kMaxK, queries_on_device ? kEnvelopeNone : kEnvelopeQuery);
        PCV_REQUIRE(!s->pending.active, "search_sharded: a pass queued by search_device_begin has not been collected");
        sync_view(s);  // (before the split into passes is chosen)
        const size_t n = (size_t)n_queries * k;
        hipStream_t st = s->ctx->stream;
        PCV_HIP(hipSetDevice(s->ctx->device));
        c->d_local.ensure(n + 1);
        c->d_gathered.ensure((n + 1) * c->world);
        c->d_merged.ensure(n + 1);
        c->pin_hits.ensure(n + 1);
        auto exchange = [&](const pcv_hit_dev* local, size_t nq, int flagged) {  // all-gather + merge + download, queued behind the local pass
            const size_t rec = nq * k + flagged;
            rccl_check(rccl().AllGather(local, c->d_gathered.p, rec * sizeof(pcv_hit_dev), /*ncclInt8*/ 0, c->comm, st),
                       "ncclAllGather");
            launch_merge(st, c->d_gathered.p, c->world, (int)nq, k, c->d_merged.p, flagged);
            PCV_HIP(hipMemcpyAsync(c->pin_hits.p, c->d_merged.p, rec * sizeof(pcv_hit_dev), hipMemcpyDeviceToHost, st));
        };
        const int qstep = pass_queries(s, pick_kernel(s, n_queries), true);  // every rank computes the same split
        std::vector<pcv_hit_dev> all(n);
        pcv_scan_stats total{};
        auto accumulate = [&] {  // every attempt starts its own statistics (device_begin)
            total.rows_scanned += s->stats.rows_scanned;
            total.bytes_algorithmic += s->stats.bytes_algorithmic;
            total.scan_ms += s->stats.scan_ms;
            total.total_ms += s->stats.total_ms;
            total.candidates += s->stats.candidates;
            total.scan_launches += s->stats.scan_launches;
            total.overflow_reruns += s->stats.overflow_reruns;
            total.speculation_reruns += s->stats.speculation_reruns;
            total.host_enqueue_ms += s->stats.host_enqueue_ms;
            total.host_wait_ms += s->stats.host_wait_ms;
            total.kernel_used = s->stats.kernel_used;
            total.bytes_streamed += s->stats.bytes_streamed;
            total.coarse_survivors += s->stats.coarse_survivors;
            total.mid_survivors += s->stats.mid_survivors;
            total.narrow_survivors += s->stats.narrow_survivors;
            total.mid_copy = s->stats.mid_copy;
            total.screening_copy = s->stats.screening_copy;
            total.screen_bits = s->stats.screen_bits;
        };
        for (int q0 = 0; q0 < n_queries; q0 += qstep) {
            const int B = std::min(qstep, n_queries - q0);
            const size_t nb = (size_t)B * k;
            // One pass: everything is queued back to back and the host waits once.  Whether a list
            // overflowed somewhere is part of the exchanged payload, so all ranks repeat (or not) together.
            for (int attempt = 0;; ++attempt) {
                device_begin(s, queries + (size_t)q0 * s->D, B, source_ids, n_sources, k, c->d_local.p, queries_on_device);
                try {
                    exchange(c->d_local.p, (size_t)B, 1);
                } catch (...) {
                    try {
                        finish_pass(s);  // collect the queued pass before reporting
                    } catch (...) {
                    }
                    throw;
                }
                finish_pass(s);  // waits for the stream (pass, all-gather, merge, download); grows this rank's lists if needed
                const bool again = c->pin_hits.p[nb].pos != 0;
                if (!again) std::memcpy(all.data() + (size_t)q0 * k, c->pin_hits.p, nb * sizeof(pcv_hit_dev));
                accumulate();
                if (!again) break;
                // Some rank's pass was incomplete (a list overflowed, or a speculative threshold did not hold — one flag
                // covers both): the repeat runs without a guess on EVERY rank, so that guesses failing on different ranks
                // in different attempts cannot use up the limit; what is left to repeat for are overflows, and each of
                // those grows the lists of the rank it happened on.
                s->spec_hold = true;
                PCV_REQUIRE(attempt < 7,
                            "search_sharded: the step is still incomplete on some rank after %d repeats (on this rank: %d candidate-list "
                            "overflows, %d speculative thresholds that did not hold)",
                            attempt + 1, total.overflow_reruns, total.speculation_reruns);
            }
        }
        s->stats = total;
        hits_to_outputs(s->metric, s->D, all.data(), n_queries, k, out_ids, out_scores, out_counts);
    });
}

pcv_status pcv_searcher_search_sharded(pcv_searcher* s, pcv_comm* c, const float* queries, int n_queries,
                                       const int64_t* source_ids, int n_sources, int k, int64_t* out_ids,
                                       float* out_scores, int* out_counts) {
    return search_sharded_impl(s, c, queries, false, n_queries, source_ids, n_sources, k, out_ids, out_scores, out_counts);
}

pcv_status pcv_searcher_search_sharded_dq(pcv_searcher* s, pcv_comm* c, const void* d_queries, int n_queries,
                                          const int64_t* source_ids, int n_sources, int k, int64_t* out_ids,
                                          float* out_scores, int* out_counts) {
    return search_sharded_impl(s, c, (const float*)d_queries, true, n_queries, source_ids, n_sources, k, out_ids, out_scores, out_counts);
}

}  // extern "C"
