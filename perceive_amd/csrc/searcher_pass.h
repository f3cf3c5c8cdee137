// searcher_pass.h — what the callers of a scan pass need (searcher_pass.cpp): the request of one pass, what a search call settles
// before its first pass, and the queue / collect pair.  Every function here is called with s->mu held; at most one pass of a
// searcher is in flight (s->pending).  row_jobs.cpp needs nothing of this file.
#pragma once
#include "searcher_internal.h"

namespace pcv {

// One pass (<= pass_queries() queries over any number of segments) as its caller asks for it: the queries and where they are,
// the selected segments, the kernel, and exactly one of three kinds of result.
struct PassRequest {
    // kDevice: `queries` is a DEVICE pointer (embeddings that never left the GPU: encode -> gather -> search of BASELINE
    // configs[4]), copied device to device behind the parameter upload.  kResident: the queries of the previous attempt are still
    // in the device's pass block; `queries` is not read.
    enum Where { kHost, kDevice, kResident };
    // kCeilings: a top-k pass among the rows that rank after one ceiling per query (scan.h, CeilRec).  kRange: every row of class
    // 1 of a ceiling, the thresholds fixed by launch_range_thresholds, range_select_kernel at the end (scan.h, RangeRec;
    // DESIGN.md §4 "Range search").
    enum Kind { kTopK, kCeilings, kRange };
    struct TopK {
        int k;
        pcv_hit_dev* d_out;     // [B][k] hits (nullptr = s->d_hits)
        bool download;          // ... into s->pin->hits as well (the survivor counts always come back that way)
        pcv_hit_dev* d_flag;    // receives the overflow record (scan.h), or nullptr
        const CeilRec* ceil;    // [B], kCeilings only
    };
    struct Range {
        const RangeRec* recs;   // [B]
        uint32_t cap, keep;     // entries per list; hits kept per sorted run
    };
    const float* queries;  // [B][D]
    Where where = kHost;
    int B;
    const SelSeg* segs;
    int nseg;
    int kernel;
    Kind kind = kTopK;
    union {
        TopK topk = {};
        Range range;
    };
    PassRequest(const float* q, int B_, const std::vector<SelSeg>& sel, int kernel_)
        : queries(q), B(B_), segs(sel.data()), nseg((int)sel.size()), kernel(kernel_) {}
    PassRequest& top_k(int k, pcv_hit_dev* d_out, bool download, pcv_hit_dev* d_flag = nullptr, const CeilRec* ceil = nullptr) {
        kind = ceil ? kCeilings : kTopK;
        topk = TopK{k, d_out, download, d_flag, ceil};
        return *this;
    }
    PassRequest& in_range(const RangeRec* recs, uint32_t cap, uint32_t keep) {
        kind = kRange;
        range = Range{recs, cap, keep};
        return *this;
    }
    int k() const { return kind == kRange ? 1 : topk.k; }  // (a range pass ranks nothing: its thresholds are fixed)
};

// the pass block in pinned memory: the parameters of the last pass queued
inline ScanParams& pass_params(const pcv_searcher* s) { return *reinterpret_cast<ScanParams*>(s->pin_pass.p); }
// What a list that needed `mx` entries is grown towards, before the caller's clamps (finish_pass and search_range clamp
// differently, on purpose): what the pass needed plus a quarter.
inline uint64_t list_need(uint32_t mx) { return (uint64_t)mx + mx / 4 + 1024; }

void ensure_workspace(pcv_searcher* s);
void enqueue_pass(pcv_searcher* s, const PassRequest& r);  // queues the pass on the context stream without waiting for it
bool finish_pass(pcv_searcher* s);                         // collects it; true: incomplete (lists grown, or a guess failed) — repeat it
void run_pass(pcv_searcher* s, PassRequest r);             // both, repeated until the pass is complete
void drop_pass_graph(pcv_searcher* s);

int pick_kernel(const pcv_searcher* s, int B);
int pass_queries(const pcv_searcher* s, int kernel, bool among_ranks = false);
enum { kEnvelopeFull = 0, kEnvelopeQuery = 1, kEnvelopeNone = 2 };  // what check_dot_envelope may look at (searcher_pass.cpp)
void check_search_args(const pcv_searcher* s, const float* queries, int n_queries, int k, const char* who, int k_max = kMaxK,
                       int envelope = kEnvelopeFull);
void check_dot_envelope(const pcv_searcher* s, const float* queries, int n_queries, const char* who, int what = kEnvelopeFull);  // dot metric: PCV_ERR_INVALID outside the f32 envelope

// What every search call settles before its first pass: the device, the selected segments, the kernel and how many queries one
// pass takes.  Nothing of the searcher changes here, so a refused kernel leaves what the caller has not touched itself.
struct SearchPlan {
    std::vector<SelSeg> segs;
    int kernel = 0;
    int qstep = 0;
};
SearchPlan plan_search(pcv_searcher* s, const int64_t* source_ids, int n_sources, int n_queries, bool among_ranks = false);
bool open_search(pcv_searcher* s, const SearchPlan& plan);
double query_norm(const float* q, int D);  // |q|, summed in f64 in feature order
void next_ceilings(const pcv_searcher* s, const float* queries, int B, const pcv_hit_dev* last, CeilRec* out);

}  // namespace pcv
