// searcher_internal.h — the Searcher handle and its building blocks as the searcher's host files share them, and what the units
// that own its rows declare for the others: searcher_store.cpp (segments and their copies), searcher_edits.cpp (changes by id)
// and searcher_views.cpp.  The pass pipeline and the search calls have headers of their own (searcher_pass.h, searcher_calls.h);
// searcher.cpp holds the C entry points, row_jobs.cpp the calls that run kernels over the stored rows.  Not part of the C ABI.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "common.h"
#include "corpus.h"
#include "scan.h"

namespace pcv {

// One device allocation of corpus rows.  Rows are appended in place while there is room (cap_rows), so a
// source that grows by many small adds stays a handful of segments; rows [scaled_rows, nrows) have been
// uploaded but not yet given their scale (they become searchable at the next finalize).
struct Segment {
    float4* blk = nullptr;
    float* scale = nullptr;
    int64_t* ids = nullptr;  // nullptr -> implicit ids id0 + row (synthetic rows)
    uint4* blk16 = nullptr;  // bf16 screening copy (scan.h), built at finalize for the rows that have their scale
    uint4* blk8 = nullptr;   // int8 screening copy + its per-row quantisation scales
    float* scale8 = nullptr;
    uint4* mid16 = nullptr;  // row-major 16-bit copy (scan.h) + its per-row scales
    float* scale16 = nullptr;
    uint32_t mid_rows = 0;   // rows the mid copy covers
    uint4* blk6 = nullptr;   // 6-bit screening copy beside the int8 one (scan.h; AUTO, large sources) + its per-block constants
    float4* scale6 = nullptr;
    uint32_t six_rows = 0;   // rows the 6-bit copy covers
    int64_t id0 = 0;
    int64_t pos0 = 0;
    uint32_t nrows = 0, cap_rows = 0, scaled_rows = 0;
    uint32_t copied_rows = 0;  // rows the screening copy covers
    uint32_t hidden_rows = 0;  // rows whose id is in the searcher's hidden set (pcv_searcher_hide_ids)
    uint32_t nblocks() const { return (nrows + kBlockRows - 1) / kBlockRows; }
};

struct Source {
    int64_t id = 0;
    std::vector<Segment> segs;
    int64_t next_implicit_id = 0;
    int64_t reserve = 0;  // rows the host announced it is going to add (pcv_searcher_reserve)
    int64_t rows() const {
        int64_t n = 0;
        for (const Segment& g : segs) n += g.nrows;
        return n;
    }
};

// A device buffer and its owner: freed when it goes out of scope.  (Whoever frees one that a queued kernel may still read
// synchronises the stream first.)
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    ~DevBuf() { release(); }
    void ensure(size_t want) {
        if (want <= n) return;
        if (p) PCV_HIP(hipFree(p));
        p = nullptr;
        n = 0;
        PCV_HIP(hipMalloc((void**)&p, want * sizeof(T)));
        n = want;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    T* hand_over() {  // the memory is the caller's from here on
        T* q = p;
        p = nullptr;
        n = 0;
        return q;
    }
};

// Its counterpart in pinned host memory (what kernels write results to and uploads are staged in).  The same rule: whoever lets
// one go that queued work may still use synchronises the stream first.
template <class T>
struct PinBuf {
    T* p = nullptr;
    size_t n = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { release(); }
    void ensure(size_t want) {
        if (want <= n) return;
        release();
        PCV_HIP(hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault));
        n = want;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    T* operator->() const { return p; }
};

// Runs `f` when the scope ends, however it ends.
template <class F>
struct AtExit {
    F f;
    ~AtExit() { f(); }
};
template <class F>
AtExit<F> at_exit(F f) {
    return {std::move(f)};
}

constexpr size_t kPassAlign = 256;
inline size_t align_up(size_t v) { return (v + kPassAlign - 1) / kPassAlign * kPassAlign; }

}  // namespace pcv

struct pcv_searcher {
    pcv_ctx* ctx = nullptr;
    int D = 0, Dp = 0, D4 = 0;
    int metric = PCV_METRIC_COSINE;
    int kernel = PCV_KERNEL_AUTO;
    int64_t shard_offset = 0;
    std::vector<pcv::Source> sources;
    uint32_t* d_max_norm_bits = nullptr;
    float max_norm = 0.0f;
    bool dirty = false;
    std::mutex mu;
    pcv_scan_stats stats{};
    pcv::DevBuf<float> d_stage;  // ingestion staging (released by finalize)
    // hidden items (pcv_searcher_hide_ids): the set, ascending, and the device scratch that applies a batch of it
    std::vector<int64_t> hidden;
    pcv::DevBuf<int64_t> d_idtab;         // the batch's hash table (scan.h: id_hash)
    pcv::DevBuf<uint32_t> d_hrows, d_hblocks, d_hcnt;
    // updated items (pcv_searcher_update_rows): the slots next to d_idtab, the matches of a segment, the (row, slot) lists of a call
    pcv::DevBuf<uint32_t> d_idslot, d_hslots, d_urows, d_uslots;

    // per-search workspace (sized for one pass of <= kMfmaQueries = 256 queries)
    pcv::DevBuf<float> d_qf32, d_qraw, d_margin, d_margin32;
    pcv::DevBuf<uint16_t> d_qbf16;
    pcv::DevBuf<int8_t> d_q8;
    pcv::DevBuf<float> d_q8c;
#ifdef PCV_STAMPS
    pcv::DevBuf<unsigned long long> d_stamps;     // diagnostic build: per-wave time stamps of the scan launch (scan_mfma8_kernel)
#endif
    pcv::DevBuf<uint32_t> d_spec;                 // speculative start thresholds of a pass (scan.h)
    bool spec_hold = false;                  // a guess failed: the repeat of that pass runs without one
    int spec_rest = 0;                       // ... and so do the next passes: 16 after a first failure, doubling up to 1024
    int spec_penalty = 0;                    //     while failures keep coming, forgotten after 4096 passes without one
    int spec_clean = 0;
    // learned part of the guess (scan.h): statistics of (k-th best - median seed slot) over the queries of one pass shape
    struct GapStats {
        int64_t n = 0;
        double mean = 0.0, m2 = 0.0;  // Welford
        double spread = 0.0;          // mean (best - median) seed slot of the same queries
        float smallest = INFINITY;
        int holdoff = 0;              // passes still to run without a learned guess after one failed
        void add(float d, float sp) {
            if (n >= 8192) {  // keep following the queries: older ones count half
                n /= 2;
                m2 /= 2.0;
            }
            n += 1;
            const double dl = d - mean;
            mean += dl / (double)n;
            m2 += dl * (d - mean);
            spread += (sp - spread) / (double)n;
            smallest = std::min(smallest, d);
        }
        void reset() {
            n = 0;
            mean = m2 = spread = 0.0;
            smallest = INFINITY;
        }
        // used only where the gaps seen are tightly concentrated (queries alike, as far as this statistic goes): then six
        // standard deviations below their mean, and no more than 0.8 of the smallest seen; otherwise no learned guess
        float gap() const {
            if (n < 128 || holdoff > 0) return NAN;
            const double sd = std::sqrt(m2 / (double)(n - 1));
            if (!(mean > 0.0) || sd > 0.15 * mean) return NAN;
            const double g = std::min(mean - 6.0 * sd, 0.8 * (double)smallest);
            return g > 0.0 ? (float)g : NAN;
        }
    } gaps;
    int64_t gap_rows = -1;
    int gap_k = 0, gap_nseg = 0;
    pcv::DevBuf<float> d_cand_s;
    pcv::DevBuf<uint32_t> d_tau, d_slots, d_cnt;
    pcv::DevBuf<uint64_t> d_cand;
    pcv::DevBuf<pcv::pcv_hit_dev> d_hits;
    // what one pass takes up: ScanParams | SegDesc[nseg] | queries[B][D], built in pinned memory and
    // sent with ONE copy into its device mirror
    pcv::PinBuf<uint8_t> pin_pass;
    pcv::DevBuf<uint8_t> d_pass;
    // what one pass brings back: written by rescore_select_kernel straight into pinned memory
    struct Pinned {
        uint32_t cnt[pcv::kMfmaQueries];
        uint32_t coarse[3 * pcv::kMfmaQueries];  // rows per query that passed the coarse screen, then those that also passed the mid screen, then
                                            // those that passed the 6-bit screen (statistics)
        float spec_base[pcv::kMfmaQueries];  // median / best seed slot per query, k-th best exact score per query (scan.h: spec_gap)
        float spec_top[pcv::kMfmaQueries];
        float kth[pcv::kMfmaQueries];
        pcv::pcv_hit_dev hits[pcv::kMfmaQueries * pcv::kMaxK];
    };
    pcv::PinBuf<Pinned> pin;
    bool state_clean = false;  // tau / slots / counters are in the state a pass starts from
    uint32_t cand_cap = 8192;
    // range search (pcv_searcher_search_range): its lists start at cand_cap and keep what a call grew them to (0: not grown);
    // range_select_kernel writes its sorted runs and their counts straight into these pinned blocks
    uint32_t range_cap = 0;
    pcv::PinBuf<pcv::pcv_hit_dev> pin_range;
    pcv::PinBuf<uint32_t> pin_range_cnt;
    // distinct results (pcv_searcher_search_distinct): what the walks of one group of queries have come to (scan.h, DistinctRec) —
    // records | kept hits | their norms | their counters, on the device and (records after every pass, the rest once) in pinned memory
    pcv::DevBuf<uint8_t> d_distinct;
    pcv::PinBuf<uint8_t> pin_distinct;
    // diverse results (pcv_searcher_search_diverse): records | result block of one group of queries on the device and in pinned
    // memory, the group's pool lists, and the scratch their rows are gathered into (scan.h, DiverseArgs; given back after the call
    // where it is large)
    pcv::DevBuf<uint8_t> d_diverse;
    pcv::PinBuf<uint8_t> pin_diverse;
    pcv::DevBuf<pcv::pcv_hit_dev> d_diverse_entries;
    pcv::DevBuf<float4> d_diverse_rows;
    // boosted results (pcv_searcher_search_boosted): records | kept hits | their boosted scores | values | ranks of one group of
    // queries, on the device and (records after every pass, the rest once) in pinned memory
    pcv::DevBuf<uint8_t> d_boost;
    pcv::PinBuf<uint8_t> pin_boost;
    // compound queries (pcv_searcher_search_compound): records | kept rows | their penalties | part scores of one group of compounds,
    // on the device and (records after every pass, the rest once) in pinned memory; and the call's tables: compound descriptors |
    // vector norms | avoided vectors
    // hipEvent time of the select steps of the most recent ranked call, and their number (pcv_searcher_last_select_stats)
    float select_ms = 0.0f;
    int32_t select_launches = 0;
    pcv::DevBuf<uint8_t> d_compound;
    pcv::PinBuf<uint8_t> pin_compound;
    pcv::DevBuf<uint8_t> d_compound_tab;
    // the id-keyed tables (corpus.h "the id-keyed tables"): keys | vals on the device, the head block beside them and the host's
    // copy of it as of the last upsert (every one ends with a synchronised download).  One type, two instances: the group table
    // (pcv_searcher_set_groups; none = kNoGroup) and the value table (pcv_searcher_set_values; none = kNoValue).  A view has
    // neither: it reads its parent's.  The scratch of a set / get call is kept for the next unless it is large.
    struct IdTable {
        const int64_t none;      // the value that means "an entry and nothing else"
        const char* const what;  // "group" / "value": for messages
        int64_t* keys = nullptr;
        int64_t* vals = nullptr;
        uint64_t slots = 0;
        pcv::GroupHead head;
        pcv::DevBuf<pcv::GroupHead> d_head;
        pcv::PinBuf<pcv::GroupHead> pin_head;
        int32_t rehashes = 0;
        float last_set_ms = 0.0f;
        pcv::DevBuf<uint32_t> d_claim, d_slot;
        pcv::DevBuf<int64_t> d_batch;
        IdTable(int64_t none_, const char* what_) : none(none_), what(what_), head{0, 0, none_, 0, 0} {}
    };
    IdTable groups{pcv::kNoGroup, "group"};
    IdTable values{pcv::kNoValue, "value"};
    // pcv_searcher_count_where: flags and tile counts of one segment, the two sums on the device and in pinned memory
    pcv::DevBuf<uint32_t> d_where_flags, d_where_tiles;
    pcv::DevBuf<int64_t> d_where_acc;
    pcv::PinBuf<int64_t> pin_where_acc;
    uint64_t values_gen = 0;  // counts the calls that changed the value table (what predicate views watch beside `gen`)
    pcv_duplicate_stats dup_stats{};  // pcv_searcher_find_duplicates (its buffers live for the call only)
    pcv_assign_stats assign_stats{};  // pcv_searcher_assign / _kmeans (likewise)
    pcv_assign_top_stats assign_top_stats{};  // pcv_searcher_assign_top (likewise)
    pcv_neighbor_stats nbr_stats{};   // pcv_searcher_neighbors (likewise)
    pcv_match_stats match_stats{};    // pcv_searcher_match (likewise)
    pcv_pair_group_stats pair_group_stats{};  // the last of pcv_searcher_neighbors_grouped, _match_grouped, _find_duplicates_grouped
    pcv_seed_stats seed_stats{};      // pcv_searcher_seeds (likewise)
    pcv_density_stats density_stats{};  // pcv_searcher_density_clusters (likewise)
    pcv_linkage_stats linkage_stats{};  // pcv_searcher_linkage_tree (likewise)
    pcv_reach_stats reach_stats{};      // pcv_searcher_reach_tree (likewise)
    pcv_moment_stats moment_stats{};  // pcv_searcher_moments / _principal_axes (likewise)
    pcv_project_stats project_stats{};  // pcv_searcher_project (likewise)
    uint32_t scan_flags = 0;  // tuning knobs: PCV_SCAN_FLAGS at creation, pcv_searcher_set_tuning
    bool fail_copy_alloc = false;  // PCV_TUNE_FAIL_COPY_ALLOC
    int mid_copy = PCV_MID_COPY_AUTO;        // pcv_searcher_set_mid_copy
    bool mid_gave_way = false;               // AUTO: building it failed, or it was dropped to make room for rows: not tried again
    bool mids_present = false;               // every row of every segment is covered by a mid copy
    int mid_hot_passes = 0;                  // AUTO: passes in a row whose coarse screen let more than kMidTrigger rows per query through
    // AUTO builds the mid copy beside the searches, on a stream of its own: the call that decides to build it queues the build
    // and goes on without the copy, and so do the calls after it until the build's event has come (a 100M-row build is tens of
    // milliseconds; round 3 ran it inside the deciding search call, 228 ms with the older kernel).  Whatever changes rows or
    // copies waits for it first (settle_mid_build).
    // The allocations of such a build are host time too (132 ms for 6 GB on the test box): a helper thread makes them and
    // queues the kernels; it works on a list of its own (MidTask) and touches no segment — settle_mid_build joins it and hands
    // the buffers to the segments.
    hipStream_t side = nullptr;
    hipEvent_t side_go = nullptr, mid_done = nullptr;
    bool mid_building = false;
    struct MidTask {
        struct Item {
            pcv::Segment* g;  // (for settle_mid_build; the helper thread does not follow it)
            const float4* blk;
            const float* scale;
            const float* scale8;
            uint32_t cap_rows, first_row, rows;
            uint4* mid16;
            float* scale16;
            bool own;  // the helper thread allocated mid16 / scale16
        };
        std::vector<Item> items;
        std::thread th;
        std::atomic<bool> queued{false};  // the helper thread is through (the kernels may still run: mid_done)
        bool joined = false, failed = false;
    };
    std::unique_ptr<MidTask> mid_task;
    int screen_copy = PCV_SCREEN_COPY_AUTO;  // pcv_searcher_set_screening_copy
    bool screen_copy_gave_way = false;       // AUTO: the copies were dropped to make room for rows
    bool six_gave_way = false;               // AUTO: the 6-bit copies were dropped to make room (rows, copies): not built again
    int copies_kind = 0;                     // 0: not every row of every segment is covered by a screening copy; 1 bf16; 2 int8
    bool wide_sharded = false;               // pcv_searcher_allow_wide_sharded_pass: the host vouches for int8 copies on every rank
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // A pass is five short launches and four event records: on small corpora its cost is the queueing.  The second time
    // a pass of the same shape comes by, its launch sequence is captured into a hipGraph and replayed from then on (what
    // changes between passes — parameters, segment table, queries — travels in the pinned block the first kernel reads).
    struct PassShape {
        int B = -1, k = 0, kernel = 0, src_kind = 0, nseg = 0, guess = 0;  // guess: the pass has the kernel that sets a speculative threshold
        uint32_t total_blocks = 0, seed_blocks = 0, flags = 0, seg0_rows = 0;
        size_t bytes = 0;
        const void *pin = nullptr, *dev = nullptr, *seg0_blk = nullptr, *seg0_scale = nullptr;
        bool operator==(const PassShape& o) const {
            return B == o.B && k == o.k && kernel == o.kernel && src_kind == o.src_kind && nseg == o.nseg && guess == o.guess && total_blocks == o.total_blocks &&
                   seed_blocks == o.seed_blocks && flags == o.flags && seg0_rows == o.seg0_rows && bytes == o.bytes && pin == o.pin &&
                   dev == o.dev && seg0_blk == o.seg0_blk && seg0_scale == o.seg0_scale;
        }
    };
    PassShape graph_shape, last_shape;
    hipGraphExec_t graph_exec = nullptr;
    int shape_seen = 0;
    float shape_fixed_ms = -1.0f;  // scan kernel's share of the pass time, of the last plainly launched pass of last_shape
    float graph_fixed_ms = 0.0f;   // ... of the shape the graph was captured for
    bool use_graph = true;
    // a pass queued by enqueue_pass and not yet collected by finish_pass
    struct Pending {
        bool active = false;
        bool done = false;  // nothing was launched (no selected rows): only the stream has to drain
        int B = 0;
        int64_t rows = 0;
        bool mid = false;  // every selected segment had its mid copy
        int src = 0;  // what the scan streamed: 0 f32 rows, 1 bf16 copies, 2 int8 copies
        int64_t stream_bytes = 0;  // ... and how many bytes of it the scan kernel has to read, padding included
        int64_t int8_bytes = 0;    // ... what the int8 copy would have been (the mid copy's trigger is the int8 screen's)
        bool six = false;          // the scan streamed the 6-bit copies
        bool replayed = false;  // launched as a graph: only the pass as a whole was timed
        bool learned = false;   // the speculative threshold had a learned part
        bool guessing = false;  // the pass ran with a speculative threshold (and sent the seed statistics home)
        bool range = false;     // a range pass (fixed thresholds; scan.h, RangeRec) ...
        uint32_t cap = 0;       // ... and the length its lists had
    } pending;
    // views (pcv_searcher_create_view; DESIGN.md §3 "Views").  As a parent: `gen` counts the calls that may have changed a search
    // result, `live_views` the views that read its rows.  As a view: the parent, the allow list (ascending, distinct) or — a
    // predicate view, pcv_searcher_create_view_where — the predicate in its place, the parent's `gen` (and, a predicate view, its
    // `values_gen`) the rows were copied at, and each row's parent position (d_ppos[view position]).
    uint64_t gen = 0;
    std::atomic<int> live_views{0};
    pcv_searcher* view_parent = nullptr;
    std::vector<int64_t> view_ids;
    bool view_by_value = false;
    pcv::WherePred view_where{0, 0, 0};
    uint64_t view_gen = 0, view_values_gen = 0;
    int32_t view_refreshes = 0;
    float view_build_ms = 0.0f;
    int64_t view_rows = 0;
    pcv::DevBuf<int64_t> d_ppos;

    pcv::Source* find_source(int64_t id) {
        for (auto& s : sources)
            if (s.id == id) return &s;
        return nullptr;
    }
    pcv::Source& get_or_add_source(int64_t id) {
        if (pcv::Source* s = find_source(id)) return *s;
        sources.emplace_back();
        sources.back().id = id;
        return sources.back();
    }
};

namespace pcv {

constexpr int64_t kStageRows = 1 << 18;                // rows per H2D staging step (384-d: 400 MB)
constexpr int64_t kMaxSegRows = (int64_t)0xffffffc0u;  // a candidate names its row in 32 bits

// the canonical order of hits
inline bool hit_better(const pcv_hit_dev& a, const pcv_hit_dev& b) {
    if (a.score != b.score) return a.score > b.score;
    return a.pos < b.pos;
}

// A copy's buffer and the buffer of its scales: both or neither (then both pointers are null and the error is returned).
// `refuse`: PCV_TUNE_FAIL_COPY_ALLOC.  Reads nothing of the searcher: the helper thread of the AUTO mid build calls it too.
template <class A, class B>
hipError_t alloc_with_scales(bool refuse, A** buf, size_t bytes, B** scales, size_t scale_bytes) {
    hipError_t e = refuse ? hipErrorOutOfMemory : hipMalloc((void**)buf, bytes);
    if (e == hipSuccess) {
        e = hipMalloc((void**)scales, scale_bytes);
        if (e != hipSuccess) (void)hipFree(*buf);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *buf = nullptr;
        *scales = nullptr;
    }
    return e;
}

// ---- searcher_store.cpp: segments and their derived copies (each is described there); the caller holds s->mu ----
struct SelSeg {
    const Segment* g;
};
std::vector<SelSeg> select_segments(pcv_searcher* s, const int64_t* source_ids, int n_sources);  // the segments with rows of the selected sources
int64_t selected_rows(const std::vector<SelSeg>& segs);
void free_segment(Segment& g);
Segment alloc_segment(pcv_searcher* s, int64_t cap_rows, bool with_ids);
void append_rows(pcv_searcher* s, Source& src, const int64_t* ids, const void* rows, int64_t n);
void assign_positions(pcv_searcher* s);
void do_finalize(pcv_searcher* s);
void extend_mid(hipStream_t st, Segment& g, int D4);
void extend_six(hipStream_t st, Segment& g, int D4);
std::vector<uint32_t> touched_blocks(const Segment& g, const std::vector<uint32_t>& rows);
void repair_copies(pcv_searcher* s, Segment& g, const uint32_t* d_rows, uint32_t nr, const uint32_t* d_blocks, uint32_t nb);
void settle_mid_build(pcv_searcher* s, bool wait);
void build_mid_copies(pcv_searcher* s, bool must);
void maybe_build_mid_copies(pcv_searcher* s);
void drop_mid_copies(pcv_searcher* s);
void drop_six_copies(pcv_searcher* s);
bool have_six_copies(const pcv_searcher* s);
void build_six_copies(pcv_searcher* s);
void drop_screening_copies(pcv_searcher* s);
void build_screening_copies(pcv_searcher* s, Source& src);
int copy_kind_wanted(const pcv_searcher* s);
void refresh_copy_state(pcv_searcher* s);
void read_max_norm(pcv_searcher* s);

// ---- searcher_edits.cpp: a batch of ids and what it finds, hides, rewrites and removes; the caller holds s->mu ----
// A batch of ids (ascending, distinct), optionally with a slot number per id (an update: the place of the id's vector in the
// call), and, once a segment with an id column needs it, its open-addressing table on the device (scan.h: id_hash): the ids in
// s->d_idtab and, with slots, each one's slot in the same cell of s->d_idslot.  kIdEmpty marks a free cell, so that id itself
// travels beside the table (has_empty, empty_slot).
struct IdBatch {
    const std::vector<int64_t>* ids = nullptr;
    const std::vector<uint32_t>* slots = nullptr;  // slots[i] belongs to ids[i]; nullptr: no slots
    bool uploaded = false, has_empty = false;
    uint32_t tmask = 0, empty_slot = 0;
};
void upload_id_batch(pcv_searcher* s, IdBatch& b);
std::pair<size_t, size_t> implicit_range(const std::vector<int64_t>& ids, const Segment& g, uint32_t r0, uint32_t r1);
std::vector<std::pair<uint32_t, uint32_t>> find_slots(pcv_searcher* s, const Segment& g, IdBatch& b);
uint32_t hide_rows_in(pcv_searcher* s, Segment& g, uint32_t r0, uint32_t r1, IdBatch& b);
int64_t apply_id_batch(pcv_searcher* s, const std::vector<int64_t>& batch, bool hide);
int64_t update_by_id(pcv_searcher* s, const int64_t* ids, const void* rows, int64_t n, const std::vector<uint32_t>& by_id,
                     std::vector<uint8_t>& found);
int64_t remove_by_id(pcv_searcher* s, const std::vector<int64_t>& batch);

// ---- searcher_views.cpp ----
void build_view(pcv_searcher* v, pcv_searcher* p);  // p->mu held
void sync_view(pcv_searcher* v);                    // every call on a view starts here (v->mu held)

}  // namespace pcv
