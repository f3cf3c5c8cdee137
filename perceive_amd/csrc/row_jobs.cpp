// row_jobs.cpp — host side of the calls that run kernels over the stored rows themselves (row_jobs.h): duplicate pairs, item labels,
// neighbours, matches, density clusters, the linkage tree, the reach tree, seeds, moments and projection, with their entry points of the C ABI.  They are one kind of call:
// select segments, open a RowsJob over them, run the call's kernels over its launch rows, bring the result down.  Everything is
// allocated for the call and given back when it ends; nothing of the searcher's pass state is touched.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <vector>

#include "common.h"
#include "row_jobs.h"
#include "searcher_internal.h"

using namespace pcv;

namespace {

// The segment table of a launch over `segs` as the row-against-row kernels read it (selfjoin_kernels.hip, assign_kernels.hip: blk,
// scale, ids, positions and the launch's block numbering; no screening copy).  out0 receives the output index of each segment's
// row 0.  -> the blocks of the launch; `rows` receives the rows of the segments.
uint32_t fill_row_table(const std::vector<SelSeg>& segs, SegDesc* tab, int64_t* out0, int64_t& rows, const char* what) {
    uint64_t blk0 = 0;
    rows = 0;
    for (size_t i = 0; i < segs.size(); ++i) {
        const Segment& g = *segs[i].g;
        tab[i] = SegDesc{};
        tab[i].blk = g.blk;
        tab[i].scale = g.scale;
        tab[i].ids = g.ids;
        tab[i].id0 = g.id0;
        tab[i].pos0 = g.pos0;
        tab[i].nrows = g.nrows;
        tab[i].nblocks = g.nblocks();
        tab[i].blk0 = (uint32_t)blk0;
        out0[i] = rows;
        blk0 += g.nblocks();
        rows += g.nrows;
        if (blk0 * kBlockRows > 0xffffffffull) PCV_FAIL(PCV_ERR_UNSUPPORTED, "%s: more than 2^32 rows in one call", what);
    }
    return (uint32_t)blk0;
}

// The segments' order by global position (row_jobs.h, NeighborArgs): ord0[i] = the launch row segment i's row 0 would have if the
// launch were in that order, order[] = the table's indices sorted by it.  A table in position order gets ord0 = blk0 * 32.
void fill_position_order(const SegDesc* tab, size_t nseg, uint32_t* ord0, uint32_t* order) {
    std::iota(order, order + nseg, 0u);
    std::sort(order, order + nseg, [&](uint32_t x, uint32_t y) { return tab[x].pos0 < tab[y].pos0; });
    uint32_t rows = 0;
    for (size_t i = 0; i < nseg; ++i) {
        ord0[order[i]] = rows;
        rows += tab[order[i]].nblocks * kBlockRows;
    }
}

// What every call of this file opens over the segments it selected: the parameter block of the launch (ScanParams | SegDesc[nseg] |
// seg_out0[nseg] | seg_ord0[nseg] | ord_seg[nseg], built in pinned memory with its device mirror), the rows' rinv / norm as selfjoin_prep_kernel leaves them, and
// the events the call times its steps with.  Only the f32 rows are read.  A call declares its own buffers BEFORE its job: the job
// then goes first, and it waits for the stream before an event is destroyed or a buffer that a queued kernel may still read is freed.
struct RowsJob {
    hipStream_t st;
    PinBuf<uint8_t> pin_p;
    DevBuf<uint8_t> d_p;
    size_t bytes = 0;
    ScanParams* p = nullptr;  // (pinned)
    const ScanParams* dp = nullptr;
    const int64_t* seg_out0 = nullptr;  // [nseg] output index of each segment's row 0 (device)
    const uint32_t* seg_ord0 = nullptr;  // [nseg], [nseg] the segments' order by global position (device; fill_position_order)
    const uint32_t* ord_seg = nullptr;
    int64_t rows = 0;
    size_t nr = 0, n_rinv = 0;  // launch rows; entries of rinv
    DevBuf<float> d_rinv;
    DevBuf<double> d_norm;
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // (the longest call brackets five steps; 6, 7: the group gather)

    // pad_blocks: the blocks of rinv behind total_blocks that must be there and zero (a tile kernel's tile_blocks; 0: none)
    // out0: the output index of each segment's row 0 where the launch order is not the output order (`match`); null: it is
    RowsJob(pcv_searcher* s, const std::vector<SelSeg>& segs, const char* what, int metric, uint32_t pad_blocks, const int64_t* out0 = nullptr)
        : st(s->ctx->stream) {
        PCV_HIP(hipSetDevice(s->ctx->device));
        const size_t nseg = segs.size();
        const size_t off_seg = align_up(sizeof(ScanParams)), off_out0 = align_up(off_seg + nseg * sizeof(SegDesc));
        const size_t off_ord = align_up(off_out0 + nseg * sizeof(int64_t));
        bytes = off_ord + 2 * nseg * sizeof(uint32_t);
        pin_p.ensure(bytes);
        d_p.ensure(bytes);
        p = new (pin_p.p) ScanParams{};
        SegDesc* tab = reinterpret_cast<SegDesc*>(pin_p.p + off_seg);
        p->total_blocks = fill_row_table(segs, tab, reinterpret_cast<int64_t*>(pin_p.p + off_out0), rows, what);
        if (out0) std::memcpy(pin_p.p + off_out0, out0, nseg * sizeof(int64_t));
        fill_position_order(tab, nseg, reinterpret_cast<uint32_t*>(pin_p.p + off_ord), reinterpret_cast<uint32_t*>(pin_p.p + off_ord) + nseg);
        seg_ord0 = reinterpret_cast<const uint32_t*>(d_p.p + off_ord);
        ord_seg = seg_ord0 + nseg;
        p->seg = reinterpret_cast<const SegDesc*>(d_p.p + off_seg);
        p->nseg = (int)segs.size();
        p->D = s->D;
        p->D4 = s->D4;
        p->metric = metric;
        dp = reinterpret_cast<const ScanParams*>(d_p.p);
        seg_out0 = reinterpret_cast<const int64_t*>(d_p.p + off_out0);
        nr = (size_t)p->total_blocks * kBlockRows;
        n_rinv = nr + (size_t)pad_blocks * kBlockRows;
        d_rinv.ensure(n_rinv);
        d_norm.ensure(nr);
    }
    ~RowsJob() {
        (void)hipStreamSynchronize(st);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    RowsJob(const RowsJob&) = delete;
    RowsJob& operator=(const RowsJob&) = delete;

    // queues the upload of the block and, between ev[0] and ev[1], the prep step; once per job, behind the memsets of the call
    void prep() {
        SelfJoinArgs a{};
        a.rinv = d_rinv.p;
        a.norm = d_norm.p;
        PCV_HIP(hipMemcpyAsync(d_p.p, pin_p.p, bytes, hipMemcpyHostToDevice, st));
        if (n_rinv > nr) PCV_HIP(hipMemsetAsync(d_rinv.p, 0, n_rinv * sizeof(float), st));
        record(0);
        launch_selfjoin_prep(st, *p, dp, a);
        record(1);
    }
    void record(int i) {  // (an event is made when the call first records it: a short call pays for no more than it uses)
        if (!ev[i]) PCV_HIP(hipEventCreate(&ev[i]));
        PCV_HIP(hipEventRecord(ev[i], st));
    }
    void wait() {
        PCV_HIP(hipStreamSynchronize(st));
        PCV_HIP(hipGetLastError());
    }
    float elapsed(int from) {
        float ms = 0.0f;
        PCV_HIP(hipEventElapsedTime(&ms, ev[from], ev[from + 1]));
        return ms;
    }
};

// The rule of the four screens for a candidate list that was too short.  `queue` queues the launches that list into room for
// `cap` entries and count everything they find, listed or not, in d_count[0]; the N counters at d_count come down into `first`.
// If the count is above `cap` — and not above `limit`, where the caller gives up with a message of its own — the list was too short:
// once more, with the room the count asks for.  The buffers `cand` grow to it (`queue` takes their addresses when it runs), `reset`
// queues what puts the counters, and whatever else the listing adds to, back where the first run found them, and the counters of the
// repeat come down into `again`.  Whether the two runs agree is the caller's to check.  The first run is timed from ev[from], which
// the caller has recorded behind the step before, to ev[from + 1]; the repeat between the two events behind ev[from], so that every
// event up to ev[from] keeps what the call recorded.
struct Listing {
    bool repeated = false;
    float ms = 0.0f, again_ms = 0.0f;
};
template <size_t N, class Queue, class Reset, class... T>
Listing list_candidates(RowsJob& job, int from, const unsigned long long* d_count, unsigned long long (&first)[N], unsigned long long (&again)[N],
                        unsigned long long& cap, uint64_t limit, Queue queue, Reset reset, DevBuf<T>&... cand) {
    auto run = [&](int e, unsigned long long* counts) {
        queue();
        job.record(e + 1);
        PCV_HIP(hipMemcpyAsync(counts, d_count, N * sizeof(unsigned long long), hipMemcpyDeviceToHost, job.st));
        job.wait();
        return job.elapsed(e);
    };
    Listing l;
    l.ms = run(from, first);
    if (first[0] <= cap || first[0] > limit) return l;
    cap = first[0];
    (cand.ensure((size_t)cap), ...);
    reset();
    job.record(from + 1);
    l.again_ms = run(from + 1, again);
    l.repeated = true;
    return l;
}

// What an entry point does once its arguments are checked: it takes the searcher's lock, refuses a call between search_device_begin
// and search_device_end, and brings a view up to date.
std::unique_lock<std::mutex> enter(pcv_searcher* s, const char* call) {
    std::unique_lock<std::mutex> lk(s->mu);
    PCV_REQUIRE(!s->pending.active, "%s: a pass queued by search_device_begin has not been collected", call);
    sync_view(s);
    return lk;
}

// The groups of a job's launch rows for the grouped calls (row_jobs.h, PairGroups; DESIGN.md §4 "Group-aware pairs"): grp, tag and the
// three counters, filled behind the job's prep step from the group table of `owner` (s itself, or the parent of a view; locked by the
// caller while the kernels may follow its pointers).  An empty or absent table makes every row a singleton.  Declared before the
// call's RowsJob, as every buffer is.
struct RowGroups {
    PairGroups a{};
    DevBuf<int64_t> d_grp;
    DevBuf<uint32_t> d_tag;
    DevBuf<unsigned long long> d_counters;
    size_t n_tag = 0;

    void open(const RowsJob& job, const pcv_searcher* owner) {
        n_tag = job.n_rinv;
        d_grp.ensure(std::max<size_t>(1, job.nr));
        d_tag.ensure(std::max<size_t>(1, n_tag));
        d_counters.ensure(kPairGroupCounters);
        a.rinv = job.d_rinv.p;
        a.keys = owner->groups.slots ? owner->groups.keys : nullptr;
        a.vals = owner->groups.vals;
        a.mask = owner->groups.slots ? (uint32_t)(owner->groups.slots - 1) : 0;
        a.side_val = owner->groups.head.side_val;
        a.grp = d_grp.p;
        a.tag = d_tag.p;
        a.counters = d_counters.p;
    }
    // before the job's prep, with the call's other memsets
    void zero(hipStream_t st) {
        PCV_HIP(hipMemsetAsync(d_tag.p, 0, std::max<size_t>(1, n_tag) * sizeof(uint32_t), st));
        PCV_HIP(hipMemsetAsync(d_counters.p, 0, kPairGroupCounters * sizeof(unsigned long long), st));
    }
    // behind the job's prep: ev[6] .. ev[7]
    void gather(RowsJob& job) {
        job.record(6);
        launch_row_groups(job.st, *job.p, job.dp, a);
        job.record(7);
    }
    // once the job has waited: the counters and the gather's time into the call's stats
    void finish(RowsJob& job, pcv_pair_group_stats& out) {
        unsigned long long c[kPairGroupCounters];
        PCV_HIP(hipMemcpy(c, d_counters.p, sizeof(c), hipMemcpyDeviceToHost));
        out.grouped_rows = (int64_t)c[kPairGroupRows];
        out.sibling_candidates = (int64_t)c[kPairGroupSiblings];
        out.collapsed = (int64_t)c[kPairGroupCollapsed];
        out.groups_ms = job.elapsed(6);
    }
};

// ---- duplicate pairs (pcv_searcher_find_duplicates; DESIGN.md §4 "Duplicate pairs") ----
// The screen may list four times the pairs a call may return before the call gives up: 2^26 entries of 8 bytes.
constexpr uint64_t kMaxJoinCandidates = (uint64_t)4 * PCV_MAX_DUPLICATE_PAIRS;
constexpr uint32_t kJoinSpanBlocks = 256;  // blocks a work item streams against its tile (12 MB at 384-d for 196 KB of tile staging)

// Three steps on the device (selfjoin_kernels.hip): norms, the bf16 screen of every tile of rows against the rows behind it, the
// canonical f64 cosine of what the screen listed.  The pairs come down once and are ordered here.  Everything the call allocates
// is its own and is given back when it ends: nothing of the searcher's pass state is touched.
// `groups` (find_duplicates_grouped): the searcher whose group table decides siblings; a pair of siblings with c >= threshold is
// counted in out_skipped instead of emitted (the rescore step; the screens know nothing of groups: one threshold serves all pairs).
void find_duplicates(pcv_searcher* s, const int64_t* source_ids, int n_sources, float threshold, int64_t max_pairs, int64_t* out_id_a,
                     int64_t* out_id_b, float* out_scores, int64_t* out_count, int64_t* out_total, const pcv_searcher* groups = nullptr,
                     int64_t* out_skipped = nullptr) {
    PCV_REQUIRE(!s->dirty, "find_duplicates: rows were added or cleared without pcv_searcher_finalize");
    s->dup_stats = pcv_duplicate_stats{};
    if (groups) s->pair_group_stats = pcv_pair_group_stats{};
    if (groups) s->pair_group_stats.flags = kGroupsSkipOwn;
    *out_count = 0;
    if (out_total) *out_total = 0;
    if (out_skipped) *out_skipped = 0;
    const int tile = mfma_pass_queries(s->Dp);
    if (tile == 0) PCV_FAIL(PCV_ERR_UNSUPPORTED, "find_duplicates: a bf16 tile of %d-d rows does not fit the LDS", s->D);
    const std::vector<SelSeg> segs = select_segments(s, source_ids, n_sources);
    if (segs.empty()) return;
    DevBuf<unsigned long long> d_cnt;
    DevBuf<uint64_t> d_cand;
    DevBuf<DupPair> d_pairs;
    RowGroups rg;
    SelfJoinArgs a{};
    a.tile_blocks = (uint32_t)tile / kBlockRows;
    RowsJob job(s, segs, "find_duplicates", s->metric, a.tile_blocks);
    hipStream_t st = job.st;
    const ScanParams& p = *job.p;
    const ScanParams* dp = job.dp;
    const int64_t rows = job.rows;

    a.span_blocks = kJoinSpanBlocks;
    while ((p.total_blocks + a.span_blocks - 1) / a.span_blocks > 65535u) a.span_blocks *= 2;  // (the grid's second dimension)
    // thr - margin in f64, rounded down: no pair with s below it has c >= thr
    a.threshold = (double)threshold;
    a.screen_threshold = std::nextafterf((float)((double)threshold - (double)selfjoin_margin(s->Dp)), -INFINITY);
    d_cnt.ensure(2);
    a.cand_cap = std::min<uint64_t>(kMaxJoinCandidates, std::max<uint64_t>(65536, 2 * (uint64_t)rows));
    d_cand.ensure(a.cand_cap);
    a.rinv = job.d_rinv.p;
    a.norm = job.d_norm.p;
    a.counters = d_cnt.p;

    unsigned long long counts[2] = {0, 0}, again[2] = {0, 0};
    PCV_HIP(hipMemsetAsync(d_cnt.p, 0, 2 * sizeof(unsigned long long), st));
    if (groups) {
        rg.open(job, groups);
        rg.zero(st);
        a.grp = rg.a.grp;
        a.skipped = rg.d_counters.p + kPairGroupSiblings;
    }
    job.prep();
    if (groups) {  // (the gather's two events lie between ev[0..1] of the prep and ev[1..2] of the screen: the screen is timed from its own)
        rg.gather(job);
        job.record(1);
    }
    const Listing screen = list_candidates(
        job, 1, d_cnt.p, counts, again, a.cand_cap, kMaxJoinCandidates,
        [&] {
            a.cand = d_cand.p;
            launch_selfjoin_screen(st, p, dp, a);
        },
        [&] { PCV_HIP(hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned long long), st)); }, d_cand);
    s->dup_stats.rows = rows;
    s->dup_stats.tile_rows = tile;
    s->dup_stats.prep_ms = job.elapsed(0) - (groups ? job.elapsed(6) : 0.0f);
    s->dup_stats.screen_ms = screen.ms;
    auto finish_groups = [&] {  // (the job has waited)
        if (!groups) return;
        rg.finish(job, s->pair_group_stats);
        if (out_skipped) *out_skipped = s->pair_group_stats.sibling_candidates;
    };
    const uint64_t n_cand = counts[0];
    s->dup_stats.candidates = (int64_t)n_cand;
    if (n_cand > kMaxJoinCandidates)
        PCV_FAIL(PCV_ERR_UNSUPPORTED,
                 "find_duplicates: the screen lists %llu candidate pairs at threshold %g, more than %llu (4 x PCV_MAX_DUPLICATE_PAIRS): raise the "
                 "threshold or join fewer rows",
                 (unsigned long long)n_cand, (double)threshold, (unsigned long long)kMaxJoinCandidates);
    if (screen.repeated) {  // (the screen lists the same pairs again)
        PCV_REQUIRE(again[0] == n_cand, "find_duplicates: the repeated screen listed %llu pairs, the first %llu", again[0], (unsigned long long)n_cand);
        s->dup_stats.reruns = 1;
        s->dup_stats.screen_ms += screen.again_ms;
    }
    if (n_cand == 0) {
        finish_groups();
        return;
    }
    a.n_cand = n_cand;
    a.pair_cap = std::min<uint64_t>(n_cand, (uint64_t)PCV_MAX_DUPLICATE_PAIRS);
    d_pairs.ensure(a.pair_cap);
    a.pairs = d_pairs.p;
    job.record(2);
    launch_selfjoin_rescore(st, p, dp, a);
    job.record(3);
    PCV_HIP(hipMemcpyAsync(counts, d_cnt.p, sizeof(counts), hipMemcpyDeviceToHost, st));
    job.wait();
    s->dup_stats.rescore_ms = job.elapsed(2);
    finish_groups();
    const uint64_t total = counts[1];
    s->dup_stats.pairs = (int64_t)total;
    if (total > (uint64_t)PCV_MAX_DUPLICATE_PAIRS)
        PCV_FAIL(PCV_ERR_UNSUPPORTED,
                 "find_duplicates: %llu duplicate pairs at threshold %g, more than PCV_MAX_DUPLICATE_PAIRS (%d): raise the threshold or join "
                 "fewer rows",
                 (unsigned long long)total, (double)threshold, (int)PCV_MAX_DUPLICATE_PAIRS);
    std::vector<DupPair> pairs((size_t)total);
    if (total > 0) PCV_HIP(hipMemcpy(pairs.data(), d_pairs.p, (size_t)total * sizeof(DupPair), hipMemcpyDeviceToHost));
    const size_t n = (size_t)std::min<uint64_t>(total, (uint64_t)max_pairs);
    auto before = [](const DupPair& x, const DupPair& y) {
        if (x.c != y.c) return x.c > y.c;
        if (x.pos_a != y.pos_a) return x.pos_a < y.pos_a;
        return x.pos_b < y.pos_b;
    };
    if (n < pairs.size())
        std::partial_sort(pairs.begin(), pairs.begin() + (std::ptrdiff_t)n, pairs.end(), before);
    else
        std::sort(pairs.begin(), pairs.end(), before);
    for (size_t i = 0; i < n; ++i) {
        out_id_a[i] = pairs[i].id_a;
        out_id_b[i] = pairs[i].id_b;
        if (out_scores) out_scores[i] = (float)pairs[i].c;
    }
    *out_count = (int64_t)n;
    if (out_total) *out_total = (int64_t)total;
}

// ---- item labels (pcv_searcher_assign, _label_sums, _kmeans; DESIGN.md §4 "Item labels") ----
constexpr uint64_t kMaxAssignCandidates = (uint64_t)1 << 28;  // (row, label) pairs the screen may list: 20 bytes each
constexpr int64_t kMaxLabelMembers = (int64_t)1 << 30;        // |t| <= 2^32 (1 + 2^-23): the int64 sums hold 2^30 of them

// Everything one call allocates, its own and given back when it ends: nothing of the searcher's pass state is touched.  The steps
// on the device are those of assign_kernels.hip; the rows' norms are selfjoin_prep_kernel's, and so are the labels' — they are
// uploaded as one small segment in the blocked layout.
struct AssignJob {
    pcv_searcher* s;
    hipStream_t st;
    int K, tile;
    PinBuf<uint8_t> pin_l;
    DevBuf<uint8_t> d_l;
    ScanParams* pl = nullptr;  // the labels
    const ScanParams* dpl = nullptr;
    float4* lab_blk = nullptr;  // pinned, blocked
    size_t bytes_l = 0;
    DevBuf<float> d_lab_rinv, d_w, d_mg, d_lb, d_cand_s, d_out_score;
    DevBuf<double> d_lab_norm;
    DevBuf<uint4> d_lab_tile;
    DevBuf<uint64_t> d_cand;
    DevBuf<unsigned long long> d_cnt, d_best_key, d_cand_key;
    DevBuf<uint32_t> d_best_lab;
    DevBuf<int32_t> d_row_label, d_out_label;
    DevBuf<int64_t> d_out_ids;
    DevBuf<long long> d_counts, d_sums;
    AssignArgs a{};
    pcv_assign_stats stats{};
    RowsJob rj;  // the rows.  The last member: it goes first, and waits for the stream before the buffers above are freed

    // the table of the rows and their norms: all that the sums need
    AssignJob(pcv_searcher* s_, const std::vector<SelSeg>& segs, int K_, int metric)
        : s(s_), st(s_->ctx->stream), K(K_), tile(mfma_pass_queries(s_->Dp)), rj(s_, segs, "assign", metric, 0) {
        a.metric = metric;
        a.seg_out0 = rj.seg_out0;
        a.K = K;
        d_row_label.ensure(rj.nr);
        a.rinv = rj.d_rinv.p;
        a.norm = rj.d_norm.p;
        a.row_label = d_row_label.p;
        PCV_HIP(hipMemsetAsync(d_row_label.p, 0xff, rj.nr * sizeof(int32_t), st));  // (-1: no label yet)
        rj.prep();
        rj.wait();
        stats.rows = rj.rows;
        stats.prep_ms = rj.elapsed(0);
    }

    // ... and what an assignment needs on top: the labels' table (a whole number of tiles), the per-row state, the candidate list
    // and the outputs
    // (m: the labels a row may keep — assign_top; the list's first room grows with it)
    void open_labels(int m = 1) {
        a.tile_blocks = (uint32_t)tile / kBlockRows;
        const uint32_t tiles = ((uint32_t)K + (uint32_t)tile - 1) / (uint32_t)tile;
        a.label_blocks = tiles * a.tile_blocks;
        const size_t slots = (size_t)a.label_blocks * kBlockRows;
        // [ScanParams][SegDesc][scale][blocked rows]
        const size_t off_lseg = align_up(sizeof(ScanParams)), off_scale = align_up(off_lseg + sizeof(SegDesc));
        const size_t off_blk = align_up(off_scale + slots * sizeof(float));
        bytes_l = off_blk + slots * s->Dp * sizeof(float);
        pin_l.ensure(bytes_l);
        d_l.ensure(bytes_l);
        std::memset(pin_l.p, 0, bytes_l);
        pl = new (pin_l.p) ScanParams{};
        SegDesc* lt = new (pin_l.p + off_lseg) SegDesc{};
        float* lscale = reinterpret_cast<float*>(pin_l.p + off_scale);
        for (int j = 0; j < K; ++j) lscale[j] = 1.0f;
        lab_blk = reinterpret_cast<float4*>(pin_l.p + off_blk);
        lt->blk = reinterpret_cast<const float4*>(d_l.p + off_blk);
        lt->scale = reinterpret_cast<const float*>(d_l.p + off_scale);
        lt->nrows = (uint32_t)K;
        lt->nblocks = a.label_blocks;
        pl->seg = reinterpret_cast<const SegDesc*>(d_l.p + off_lseg);
        pl->nseg = 1;
        pl->total_blocks = a.label_blocks;
        pl->D = s->D;
        pl->D4 = s->D4;
        dpl = reinterpret_cast<const ScanParams*>(d_l.p);
        a.lab_blk = lt->blk;

        const size_t nr = rj.nr;
        d_lb.ensure(nr);
        d_best_key.ensure(nr);
        d_best_lab.ensure(nr);
        d_lab_rinv.ensure(slots);
        d_lab_norm.ensure(slots);
        d_w.ensure(slots);
        d_mg.ensure(slots);
        d_lab_tile.ensure(slots * (size_t)(s->Dp / 8));
        d_cnt.ensure(2);
        d_out_label.ensure((size_t)rj.rows);
        d_out_score.ensure((size_t)rj.rows);
        d_out_ids.ensure((size_t)rj.rows);
        d_counts.ensure((size_t)K);
        a.cand_cap = std::min<uint64_t>(kMaxAssignCandidates, std::max<uint64_t>(65536, 4 * (uint64_t)m * (uint64_t)rj.rows));
        d_cand.ensure(a.cand_cap);
        d_cand_s.ensure(a.cand_cap);
        a.lab_rinv = d_lab_rinv.p;
        a.lab_norm = d_lab_norm.p;
        a.lab_tile = d_lab_tile.p;
        a.w = d_w.p;
        a.mg = d_mg.p;
        a.lb = d_lb.p;
        a.cand = d_cand.p;
        a.cand_s = d_cand_s.p;
        a.counters = d_cnt.p;
        a.best_key = d_best_key.p;
        a.best_lab = d_best_lab.p;
        a.out_label = d_out_label.p;
        a.out_score = d_out_score.p;
        a.out_ids = d_out_ids.p;
        a.out_counts = d_counts.p;
        a.margin = selfjoin_margin(s->Dp);
        // a workgroup stages a whole tile for its span: spans of two per CU, and not so short that the staging shows
        const uint32_t per = (rj.p->total_blocks + 2 * (uint32_t)s->ctx->num_cus - 1) / (2 * (uint32_t)std::max(1, s->ctx->num_cus));
        a.span_blocks = std::max<uint32_t>(32, (per + 7) / 8 * 8);
        stats.tile_labels = tile;
        stats.label_tiles = (int32_t)tiles;
    }

    // queues, between ev[0] and ev[1], what every assignment with labels[K][D] (host) starts with: the labels' upload, their norms and
    // screening constants, the rows' state
    void queue_prep(const float* labels) {
        const int D = s->D, D4 = s->D4;
        for (int j = 0; j < K; ++j) {
            float* dst = reinterpret_cast<float*>(lab_blk + (size_t)(j >> 5) * D4 * 32 + (j & 31));  // piece f of label j: dst + f * 128 floats
            for (int d = 0; d < D; ++d) dst[(size_t)(d >> 2) * 128 + (d & 3)] = labels[(size_t)j * D + d];
        }
        SelfJoinArgs prep{};
        prep.rinv = d_lab_rinv.p;
        prep.norm = d_lab_norm.p;
        PCV_HIP(hipMemcpyAsync(d_l.p, pin_l.p, bytes_l, hipMemcpyHostToDevice, st));
        PCV_HIP(hipMemsetAsync(d_cnt.p, 0, 2 * sizeof(unsigned long long), st));
        PCV_HIP(hipMemsetAsync(d_counts.p, 0, (size_t)K * sizeof(long long), st));
        rj.record(0);
        launch_selfjoin_prep(st, *pl, dpl, prep);
        launch_assign_labels(st, *rj.p, a);
        launch_assign_begin(st, *rj.p, rj.dp, a);
        rj.record(1);
    }

    // one assignment with labels[K][D] (host): row_label, the outputs on the device, counters[1] = rows whose label changed
    uint64_t assign(const float* labels) {
        unsigned long long counts[2] = {0, 0}, again[2] = {0, 0};
        queue_prep(labels);
        const Listing screen = list_candidates(
            rj, 1, d_cnt.p, counts, again, a.cand_cap, kMaxAssignCandidates,
            [&] {
                a.cand = d_cand.p;
                a.cand_s = d_cand_s.p;
                for (uint32_t t = 0; t < (uint32_t)stats.label_tiles; ++t) {
                    a.tile = t;
                    launch_assign_screen(st, *rj.p, rj.dp, a);
                }
            },
            [&] { PCV_HIP(hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned long long), st)); }, d_cand, d_cand_s);
        stats.prep_ms += rj.elapsed(0);
        stats.screen_ms += screen.ms;
        uint64_t n_cand = counts[0];
        stats.candidates = (int64_t)n_cand;
        if (n_cand > kMaxAssignCandidates)
            PCV_FAIL(PCV_ERR_UNSUPPORTED, "assign: the screen lists %llu (row, label) candidates, more than %llu: fewer or less alike labels, or fewer rows",
                     (unsigned long long)n_cand, (unsigned long long)kMaxAssignCandidates);
        if (screen.repeated) {  // (the bounds the first run left only shorten the list)
            PCV_REQUIRE(again[0] <= n_cand, "assign: the repeated screen listed %llu candidates, the first %llu", again[0], (unsigned long long)n_cand);
            n_cand = again[0];
            stats.reruns += 1;
            stats.screen_ms += screen.again_ms;
        }
        a.n_cand = n_cand;
        d_cand_key.ensure((size_t)std::max<uint64_t>(1, n_cand));
        a.cand_key = d_cand_key.p;
        rj.record(2);
        launch_assign_rescore(st, *rj.p, rj.dp, a);
        launch_assign_finish(st, *rj.p, rj.dp, a);
        rj.record(3);
        PCV_HIP(hipMemcpyAsync(counts, d_cnt.p, sizeof(counts), hipMemcpyDeviceToHost, st));
        rj.wait();
        stats.rescore_ms += rj.elapsed(2);
        return counts[1];
    }

    // the integer sums of the labels in row_label -> host [K][Dp] and the members per label
    void sums(std::vector<long long>& S, std::vector<long long>& members) {
        const size_t n = (size_t)K * s->Dp;
        d_sums.ensure(n + (size_t)K);
        a.sums = d_sums.p;
        a.sum_counts = d_sums.p + n;
        S.resize(n);
        members.resize((size_t)K);
        PCV_HIP(hipMemsetAsync(d_sums.p, 0, (n + (size_t)K) * sizeof(long long), st));
        launch_label_sums(st, *rj.p, rj.dp, a);
        PCV_HIP(hipMemcpyAsync(S.data(), d_sums.p, n * sizeof(long long), hipMemcpyDeviceToHost, st));
        PCV_HIP(hipMemcpyAsync(members.data(), d_sums.p + n, (size_t)K * sizeof(long long), hipMemcpyDeviceToHost, st));
        rj.wait();
    }

    void download(int32_t* out_label, float* out_score, int64_t* out_ids, int64_t* out_counts) {
        const size_t n = (size_t)rj.rows;
        PCV_HIP(hipMemcpy(out_label, d_out_label.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (out_score) PCV_HIP(hipMemcpy(out_score, d_out_score.p, n * sizeof(float), hipMemcpyDeviceToHost));
        if (out_ids) PCV_HIP(hipMemcpy(out_ids, d_out_ids.p, n * sizeof(int64_t), hipMemcpyDeviceToHost));
        if (out_counts) PCV_HIP(hipMemcpy(out_counts, d_counts.p, (size_t)K * sizeof(int64_t), hipMemcpyDeviceToHost));
    }
};

void check_labels(pcv_searcher* s, const float* labels, int K, const char* what) {
    for (size_t i = 0, e = (size_t)K * s->D; i < e; ++i)
        PCV_REQUIRE(std::isfinite(labels[i]), "%s: label %d has a NaN or Inf at feature %d", what, (int)(i / s->D), (int)(i % s->D));
}

// assign (max_iters = 0, the searcher's metric, no centroids) and k-means (cosine); the caller has checked the arguments
void assign_or_kmeans(pcv_searcher* s, const char* what, const float* init, int K, int max_iters, int metric, const int64_t* source_ids, int n_sources,
                      int64_t capacity, float* out_centroids, int32_t* out_label, float* out_score, int64_t* out_ids, int64_t* out_counts,
                      int32_t* out_iters, int64_t* out_moved, int64_t* out_n) {
    PCV_REQUIRE(!s->dirty, "%s: rows were added or cleared without pcv_searcher_finalize", what);
    check_labels(s, init, K, what);
    const std::vector<SelSeg> segs = select_segments(s, source_ids, n_sources);
    const int64_t n = selected_rows(segs);
    *out_n = n;
    if (out_iters) *out_iters = 0;
    if (out_label == nullptr && capacity == 0) return;  // the count alone
    PCV_REQUIRE(capacity >= n, "%s: the outputs have room for %lld rows, the selected sources have %lld", what, (long long)capacity, (long long)n);
    s->assign_stats = pcv_assign_stats{};
    if (mfma_pass_queries(s->Dp) == 0) PCV_FAIL(PCV_ERR_UNSUPPORTED, "%s: a bf16 tile of %d-d labels does not fit the LDS", what, s->D);
    const size_t KD = (size_t)K * s->D;
    if (out_centroids) std::memcpy(out_centroids, init, KD * sizeof(float));
    if (out_counts) std::fill(out_counts, out_counts + K, (int64_t)0);
    if (out_moved) out_moved[0] = 0;
    if (n == 0) return;
    AssignJob job(s, segs, K, metric);
    job.open_labels();
    const auto keep_stats = at_exit([&] { s->assign_stats = job.stats; });
    std::vector<float> cent(init, init + KD);
    std::vector<long long> S, members;
    int updates = 0;
    while (true) {
        const uint64_t moved = job.assign(cent.data());
        if (out_moved) out_moved[updates] = (int64_t)moved;
        if (moved == 0 || updates == max_iters) break;
        job.sums(S, members);
        for (int j = 0; j < K; ++j) {
            if (members[(size_t)j] > kMaxLabelMembers)
                PCV_FAIL(PCV_ERR_UNSUPPORTED, "%s: label %d has %lld members, more than 2^30", what, j, members[(size_t)j]);
            if (members[(size_t)j] == 0) continue;  // (keeps its vector)
            for (int d = 0; d < s->D; ++d) cent[(size_t)j * s->D + d] = (float)((double)S[(size_t)j * s->Dp + d] * 0x1p-32);
        }
        ++updates;
    }
    if (out_iters) *out_iters = updates;
    if (out_centroids) std::memcpy(out_centroids, cent.data(), KD * sizeof(float));
    job.download(out_label, out_score, out_ids, out_counts);
}

// ---- top-m labels (pcv_searcher_assign_top; DESIGN.md §4 "Top-m labels") ----
// An assignment's job with the two-pass screen in place of the carried bound: per label tile a bound pass and the merge of its column
// maxima, then the list passes against the final thresholds, the f64 step into per-row stretches and the selection of the m best.
struct AssignTopJob {
    DevBuf<float> d_colmax, d_topm, d_scores;
    DevBuf<uint32_t> d_row_cnt, d_row_off, d_sorted_lab;
    DevBuf<unsigned long long> d_sorted_key;
    DevBuf<int32_t> d_labels, d_count;
    AssignTopArgs x{};
    pcv_assign_top_stats stats{};
    AssignJob base;  // the last member: it goes first, and waits for the stream before the buffers above are freed

    AssignTopJob(pcv_searcher* s, const std::vector<SelSeg>& segs, int K, int m, float min_score) : base(s, segs, K, s->metric) {
        base.open_labels(m);
        const size_t nr = base.rj.nr, rows = (size_t)base.rj.rows;
        d_colmax.ensure(nr * 32);
        d_topm.ensure(nr * kMaxTopLabels);
        d_row_cnt.ensure(nr);
        d_row_off.ensure(nr + 1);
        d_labels.ensure(rows * (size_t)m);
        d_scores.ensure(rows * (size_t)m);
        d_count.ensure(rows);
        x.a = base.a;
        x.colmax = d_colmax.p;
        x.topm = d_topm.p;
        x.row_cnt = d_row_cnt.p;
        x.row_off = d_row_off.p;
        x.out_labels = d_labels.p;
        x.out_scores = d_scores.p;
        x.out_count = d_count.p;
        x.out_label_rows = base.d_counts.p;
        x.min_score = min_score;
        x.m = m;
        stats.rows = base.stats.rows;
        stats.m = m;
        stats.label_tiles = base.stats.label_tiles;
        stats.tile_labels = base.stats.tile_labels;
        stats.prep_ms = base.stats.prep_ms;
    }

    void run(const float* labels) {
        RowsJob& rj = base.rj;
        hipStream_t st = base.st;
        unsigned long long counts[1] = {0}, again[1] = {0};
        base.queue_prep(labels);
        PCV_HIP(hipMemsetAsync(d_row_cnt.p, 0, rj.nr * sizeof(uint32_t), st));
        for (uint32_t t = 0; t < (uint32_t)stats.label_tiles; ++t) {
            x.a.tile = t;
            launch_assign_top_bound(st, *rj.p, rj.dp, x);
            launch_assign_top_merge(st, *rj.p, x);
        }
        rj.record(2);
        const Listing list = list_candidates(
            rj, 2, base.d_cnt.p, counts, again, x.a.cand_cap, kMaxAssignCandidates,
            [&] {
                x.a.cand = base.d_cand.p;
                x.a.cand_s = base.d_cand_s.p;
                for (uint32_t t = 0; t < (uint32_t)stats.label_tiles; ++t) {
                    x.a.tile = t;
                    launch_assign_top_list(st, *rj.p, rj.dp, x);
                }
            },
            [&] { PCV_HIP(hipMemsetAsync(base.d_cnt.p, 0, sizeof(unsigned long long), st)); }, base.d_cand, base.d_cand_s);
        stats.prep_ms += rj.elapsed(0);
        stats.bound_ms = rj.elapsed(1);
        stats.screen_ms = list.ms;
        const uint64_t n_cand = counts[0];
        stats.candidates = (int64_t)n_cand;
        if (n_cand > kMaxAssignCandidates)
            PCV_FAIL(PCV_ERR_UNSUPPORTED, "assign_top: the screen lists %llu (row, label) candidates, more than %llu: fewer or less alike labels, a smaller m, or fewer rows",
                     (unsigned long long)n_cand, (unsigned long long)kMaxAssignCandidates);
        if (list.repeated) {  // (the thresholds were final before the first run: the same list)
            PCV_REQUIRE(again[0] == n_cand, "assign_top: the repeated list pass found %llu candidates, the first %llu", again[0], (unsigned long long)n_cand);
            stats.reruns += 1;
            stats.screen_ms += list.again_ms;
        }
        x.a.n_cand = n_cand;
        d_sorted_key.ensure((size_t)std::max<uint64_t>(1, n_cand));
        d_sorted_lab.ensure((size_t)std::max<uint64_t>(1, n_cand));
        x.sorted_key = d_sorted_key.p;
        x.sorted_lab = d_sorted_lab.p;
        rj.record(4);
        launch_assign_top_rescore(st, *rj.p, rj.dp, x);
        rj.record(5);
        launch_assign_top_select(st, *rj.p, rj.dp, x);
        rj.record(6);
        rj.wait();
        stats.rescore_ms = rj.elapsed(4);
        stats.select_ms = rj.elapsed(5);
    }

    void download(int32_t* out_labels, float* out_scores, int64_t* out_ids, int32_t* out_counts, int64_t* out_label_rows) {
        const size_t n = (size_t)base.rj.rows, m = (size_t)x.m;
        PCV_HIP(hipMemcpy(out_labels, d_labels.p, n * m * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (out_scores) PCV_HIP(hipMemcpy(out_scores, d_scores.p, n * m * sizeof(float), hipMemcpyDeviceToHost));
        if (out_ids) PCV_HIP(hipMemcpy(out_ids, base.d_out_ids.p, n * sizeof(int64_t), hipMemcpyDeviceToHost));
        PCV_HIP(hipMemcpy(out_counts, d_count.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (out_label_rows) PCV_HIP(hipMemcpy(out_label_rows, base.d_counts.p, (size_t)base.K * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) stats.listed += out_counts[i];
    }
};

// the caller has checked the arguments
void assign_top(pcv_searcher* s, const float* labels, int K, int m, float min_score, const int64_t* source_ids, int n_sources, int64_t capacity,
                int32_t* out_labels, float* out_scores, int64_t* out_ids, int32_t* out_counts, int64_t* out_label_rows, int64_t* out_n) {
    PCV_REQUIRE(!s->dirty, "assign_top: rows were added or cleared without pcv_searcher_finalize");
    check_labels(s, labels, K, "assign_top");
    const std::vector<SelSeg> segs = select_segments(s, source_ids, n_sources);
    const int64_t n = selected_rows(segs);
    *out_n = n;
    if (out_labels == nullptr && capacity == 0) return;  // the count alone
    PCV_REQUIRE(capacity >= n, "assign_top: the outputs have room for %lld rows, the selected sources have %lld", (long long)capacity, (long long)n);
    s->assign_top_stats = pcv_assign_top_stats{};
    s->assign_top_stats.m = m;
    if (mfma_pass_queries(s->Dp) == 0) PCV_FAIL(PCV_ERR_UNSUPPORTED, "assign_top: a bf16 tile of %d-d labels does not fit the LDS", s->D);
    if (out_label_rows) std::fill(out_label_rows, out_label_rows + K, (int64_t)0);
    if (n == 0) return;
    AssignTopJob job(s, segs, K, m, min_score);
    const auto keep_stats = at_exit([&] { s->assign_top_stats = job.stats; });
    job.run(labels);
    job.download(out_labels, out_scores, out_ids, out_counts, out_label_rows);
}

void label_sums(pcv_searcher* s, const int64_t* source_ids, int n_sources, const int32_t* labels, int64_t n, int K, int64_t* out_sums,
                int64_t* out_counts) {
    PCV_REQUIRE(!s->dirty, "label_sums: rows were added or cleared without pcv_searcher_finalize");
    const std::vector<SelSeg> segs = select_segments(s, source_ids, n_sources);
    PCV_REQUIRE(n == selected_rows(segs), "label_sums: %lld labels for %lld rows of the selected sources", (long long)n, (long long)selected_rows(segs));
    for (int64_t i = 0; i < n; ++i) PCV_REQUIRE(labels[i] < K, "label_sums: row %lld has label %d of %d", (long long)i, labels[i], K);
    std::fill(out_sums, out_sums + (size_t)K * s->D, (int64_t)0);
    if (out_counts) std::fill(out_counts, out_counts + K, (int64_t)0);
    if (n == 0) return;
    AssignJob job(s, segs, K, PCV_METRIC_COSINE);  // (the sums need no label tile: any dimension)
    std::vector<int32_t> by_row(job.rj.nr, -1);
    size_t lr = 0;
    int64_t at = 0;
    for (const SelSeg& g : segs) {
        for (uint32_t r = 0; r < g.g->nrows; ++r) by_row[lr + r] = labels[at + r] < 0 ? -1 : labels[at + r];
        lr += (size_t)g.g->nblocks() * kBlockRows;
        at += g.g->nrows;
    }
    PCV_HIP(hipMemcpy(job.d_row_label.p, by_row.data(), by_row.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    std::vector<long long> S, members;
    job.sums(S, members);
    for (int j = 0; j < K; ++j) {
        if (members[(size_t)j] > kMaxLabelMembers) PCV_FAIL(PCV_ERR_UNSUPPORTED, "label_sums: label %d has %lld members, more than 2^30", j, members[(size_t)j]);
        for (int d = 0; d < s->D; ++d) out_sums[(size_t)j * s->D + d] = (int64_t)S[(size_t)j * s->Dp + d];
        if (out_counts) out_counts[j] = (int64_t)members[(size_t)j];
    }
}

// ---- item neighbours (pcv_searcher_neighbors; DESIGN.md §4 "Item neighbours") ----
constexpr uint64_t kMaxNeighborCandidates = (uint64_t)1 << 30;  // directed (owner, partner) pairs the list pass may leave: 20 bytes each
constexpr uint32_t kNeighborWalkBlocks = 256;  // sampled blocks a workgroup streams against its tile (kJoinSpanBlocks)

// sampled blocks one workgroup of a walking screen streams against its tile: the grid's second dimension holds 65535 walks
uint32_t walk_blocks(uint32_t TB) {
    uint32_t walk_len = kNeighborWalkBlocks;
    while ((TB + walk_len - 1) / walk_len > 65535u) walk_len *= 2;
    return walk_len;
}

// The sample of the neighbours' bound pass over PB partner blocks and its spans (DESIGN.md §4 "Item neighbours", measurement): no
// result depends on them, only the list's length.  No partner block: one empty span.
void neighbor_sample(uint32_t PB, int k, uint32_t& stride, uint32_t& span_len, uint32_t& spans) {
    stride = std::min<uint32_t>(4, std::max<uint32_t>(1, PB / (uint32_t)std::max(64, 4 * k)));
    const uint32_t sampled = std::max<uint32_t>(1, (PB + stride - 1) / stride);
    const uint32_t want_spans = std::min<uint32_t>(sampled, std::min<uint32_t>(kMaxNeighborSpans, (uint32_t)std::max(64, 8 * k)));
    span_len = (sampled + want_spans - 1) / want_spans;
    spans = (sampled + span_len - 1) / span_len;
}

// The rescored candidates of every owner row's k best partners, as `neighbors`, `match` and the core step of `reach_tree` get them:
// the sample, the buffers and their wiring, then bound pass, thresholds, list pass with the rerun rule, and the rescore that leaves
// sorted_key / sorted_row / row_off.  The owners are the launch blocks [owner_block0, total_blocks), the partners [0, partner_blocks):
// `neighbors` and `reach_tree` open it over the whole launch (open), `match` over its two ranges (open_ranges).  Declared before the call's RowsJob, as every buffer is.  The counter of the list pass is the caller's, and so
// are the messages: `list` hands back what it counted.
struct NeighborPlan {
    NeighborArgs a{};
    DevBuf<float> d_thr;
    DevBuf<uint32_t> d_span_max, d_cnt_off, d_sorted_row;
    DevBuf<unsigned long long> d_sorted_key;
    DevBuf<uint64_t> d_cand;
    DevBuf<unsigned long long> d_span_max64;  // the grouped calls: the 64-bit span images, the partners' groups beside sorted_row
    DevBuf<int64_t> d_sorted_grp;
    size_t nr = 0, n_pad = 0, n_span_max = 0;

    // The mode, before open: off unless this is called (`neighbors`, `match` and the core step of `reach_tree` never do: their launches
    // are the plain ones).  The rescore and select steps then carry the partners' groups; flags != 0 gives the bound pass and the
    // thresholds their grouped form, over span images of 8 bytes instead of 4.
    void with_groups(const RowGroups& rg, uint32_t flags) {
        a.grp = rg.a.grp;
        a.tag = rg.a.tag;
        a.gcounters = rg.a.counters;
        a.group_flags = flags;
    }
    void open(const RowsJob& job, uint32_t tile_blocks, int k, float margin, unsigned long long* counter) {
        open_ranges(job, tile_blocks, k, margin, counter, 0, job.p->total_blocks, -1.0f, job.rows);
    }
    // owner_rows: the rows of the owners' segments, which size the first candidate list
    void open_ranges(const RowsJob& job, uint32_t tile_blocks, int k, float margin, unsigned long long* counter, uint32_t owner_block0,
                     uint32_t partner_blocks, float min_score, int64_t owner_rows) {
        const uint32_t TB = job.p->total_blocks;
        a.tile_blocks = tile_blocks;
        a.k = k;
        a.margin = margin;
        a.min_score = min_score;
        a.owner_block0 = owner_block0;
        a.partner_blocks = partner_blocks;
        neighbor_sample(partner_blocks, k, a.stride, a.span_len, a.spans);
        a.walk_len = walk_blocks(partner_blocks);
        nr = job.nr;
        n_pad = job.n_rinv;
        n_span_max = (size_t)a.spans * (size_t)(TB - owner_block0) * kBlockRows;
        d_thr.ensure(n_pad);
        if (a.group_flags != 0) {
            d_span_max64.ensure(std::max<size_t>(1, n_span_max));
            a.span_max64 = d_span_max64.p;
        }
        d_span_max.ensure(a.group_flags != 0 ? 1 : std::max<size_t>(1, n_span_max));
        d_cnt_off.ensure(2 * nr + 1);
        a.cand_cap = std::min<uint64_t>(kMaxNeighborCandidates, std::max<uint64_t>(65536, (uint64_t)32 * (uint64_t)k * (uint64_t)owner_rows));
        d_cand.ensure(a.cand_cap);
        a.rinv = job.d_rinv.p;
        a.thr = d_thr.p;
        a.norm = job.d_norm.p;
        a.span_max = d_span_max.p;
        a.row_cnt = d_cnt_off.p;
        a.row_off = d_cnt_off.p + nr;
        a.counters = counter;
        a.seg_out0 = job.seg_out0;
        a.seg_ord0 = job.seg_ord0;
        a.ord_seg = job.ord_seg;
    }
    void zero(hipStream_t st) {
        PCV_HIP(hipMemsetAsync(d_thr.p, 0, n_pad * sizeof(float), st));
        if (n_span_max && a.group_flags == 0) PCV_HIP(hipMemsetAsync(d_span_max.p, 0, n_span_max * sizeof(uint32_t), st));
        if (n_span_max && a.group_flags != 0) PCV_HIP(hipMemsetAsync(d_span_max64.p, 0, n_span_max * sizeof(unsigned long long), st));
        PCV_HIP(hipMemsetAsync(d_cnt_off.p, 0, (2 * nr + 1) * sizeof(uint32_t), st));
    }
    // bound pass and thresholds up to ev[2], then the list pass over every partner block, timed from there
    Listing list(RowsJob& job, unsigned long long (&count)[1], unsigned long long (&again)[1]) {
        launch_neighbors_bound(job.st, *job.p, job.dp, a);
        launch_neighbors_threshold(job.st, *job.p, a);
        job.record(2);
        a.stride = 1;  // the list pass: every block
        return list_candidates(
            job, 2, a.counters, count, again, a.cand_cap, kMaxNeighborCandidates,
            [&] {
                a.cand = d_cand.p;
                launch_neighbors_list(job.st, *job.p, job.dp, a);
            },
            [&] { PCV_HIP(hipMemsetAsync(a.counters, 0, sizeof(unsigned long long), job.st)); }, d_cand);
    }
    // ev[3], then candidates per owner, their offsets and the f64 cosine of each
    void rescore(RowsJob& job, uint64_t n_cand) {
        a.n_cand = n_cand;
        d_sorted_key.ensure((size_t)std::max<uint64_t>(1, n_cand));
        d_sorted_row.ensure((size_t)std::max<uint64_t>(1, n_cand));
        a.sorted_key = d_sorted_key.p;
        a.sorted_row = d_sorted_row.p;
        if (a.grp != nullptr) {
            d_sorted_grp.ensure((size_t)std::max<uint64_t>(1, n_cand));
            a.sorted_grp = d_sorted_grp.p;
        }
        job.record(3);
        launch_neighbors_rescore(job.st, *job.p, job.dp, a);
    }
    void release() {
        d_thr.release();
        d_span_max.release();
        d_cnt_off.release();
        d_sorted_key.release();
        d_sorted_row.release();
        d_cand.release();
        d_span_max64.release();
        d_sorted_grp.release();
    }
};

// Prep, bound pass, thresholds, list pass, rescore, select (neighbors_kernels.hip).  Everything the call allocates is its own and
// is given back when it ends: nothing of the searcher's pass state is touched, and only the f32 rows are read.
// `groups` (neighbors_grouped): the searcher whose group table the call reads, with the PCV_GROUPS_* flags and the partners' groups.
void neighbors(pcv_searcher* s, const int64_t* source_ids, int n_sources, int k, int64_t capacity, int64_t* out_ids, int64_t* out_neighbor_ids,
               float* out_scores, int32_t* out_counts, int64_t* out_rows, const pcv_searcher* groups = nullptr, uint32_t flags = 0,
               int64_t* out_groups = nullptr) {
    PCV_REQUIRE(!s->dirty, "neighbors: rows were added or cleared without pcv_searcher_finalize");
    PCV_REQUIRE(s->shard_offset == 0, "neighbors: a sharded searcher (set_shard_offset) is not supported");
    const std::vector<SelSeg> segs = select_segments(s, source_ids, n_sources);
    const int64_t n = selected_rows(segs);
    *out_rows = n;
    if (out_ids == nullptr && capacity == 0) return;  // the count alone
    PCV_REQUIRE(capacity >= n, "neighbors: the outputs have room for %lld rows, the selected sources have %lld", (long long)capacity, (long long)n);
    s->nbr_stats = pcv_neighbor_stats{};
    if (groups) s->pair_group_stats = pcv_pair_group_stats{};
    const int tile = mfma_pass_queries(s->Dp);
    if (tile == 0) PCV_FAIL(PCV_ERR_UNSUPPORTED, "neighbors: a bf16 tile of %d-d rows does not fit the LDS", s->D);
    if (groups) {
        s->pair_group_stats.flags = flags;
        s->pair_group_stats.bound_tile_rows = flags != 0 ? std::min(tile, 2 * (int)kBlockRows) : tile;
    }
    if (n == 0) return;
    NeighborPlan plan;
    RowGroups rg;
    DevBuf<float> d_out_score;
    DevBuf<unsigned long long> d_cnt;
    DevBuf<int64_t> d_out_ids, d_out_nbr, d_out_grp;
    DevBuf<int32_t> d_out_count;
    RowsJob job(s, segs, "neighbors", PCV_METRIC_COSINE, (uint32_t)tile / kBlockRows);
    hipStream_t st = job.st;
    const ScanParams& p = *job.p;
    const ScanParams* dp = job.dp;
    const int64_t rows = job.rows;

    d_cnt.ensure(1);
    if (groups) {
        rg.open(job, groups);
        plan.with_groups(rg, flags);
    }
    plan.open(job, (uint32_t)tile / kBlockRows, k, selfjoin_margin(s->Dp), d_cnt.p);
    NeighborArgs& a = plan.a;
    d_out_ids.ensure((size_t)rows);
    d_out_nbr.ensure((size_t)rows * k);
    d_out_score.ensure((size_t)rows * k);
    d_out_count.ensure((size_t)rows);
    a.out_ids = d_out_ids.p;
    a.out_nbr = d_out_nbr.p;
    a.out_score = d_out_score.p;
    a.out_count = d_out_count.p;
    if (groups) {
        d_out_grp.ensure((size_t)rows * k);
        a.out_grp = d_out_grp.p;
    }

    pcv_neighbor_stats& stats = s->nbr_stats;
    stats.rows = rows;
    stats.k = k;
    stats.tile_rows = tile;
    stats.sample_stride = (int32_t)a.stride;
    stats.spans = (int32_t)a.spans;

    unsigned long long count[1] = {0}, again[1] = {0};
    plan.zero(st);
    PCV_HIP(hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned long long), st));
    if (groups) rg.zero(st);
    job.prep();
    if (groups) {  // (ev[1] again behind the gather: the bound pass is timed from there, the prep up to the gather)
        rg.gather(job);
        job.record(1);
    }
    const Listing list = plan.list(job, count, again);
    stats.prep_ms = job.elapsed(0) - (groups ? job.elapsed(6) : 0.0f);
    stats.bound_ms = job.elapsed(1);
    stats.screen_ms = list.ms;
    const uint64_t n_cand = count[0];
    stats.candidates = (int64_t)n_cand;
    if (n_cand > kMaxNeighborCandidates)
        PCV_FAIL(PCV_ERR_UNSUPPORTED, "neighbors: the list pass leaves %llu candidates for k = %d, more than %llu: ask for fewer neighbours or fewer rows",
                 (unsigned long long)n_cand, k, (unsigned long long)kMaxNeighborCandidates);
    if (list.repeated) {  // (the pass lists the same pairs again)
        PCV_REQUIRE(again[0] == n_cand, "neighbors: the repeated list pass left %llu candidates, the first %llu", again[0], (unsigned long long)n_cand);
        stats.reruns = 1;
        stats.screen_ms += list.again_ms;
    }
    plan.rescore(job, n_cand);
    job.record(4);
    launch_neighbors_select(st, p, dp, a);
    job.record(5);
    job.wait();
    stats.rescore_ms = job.elapsed(3);
    stats.select_ms = job.elapsed(4);
    PCV_HIP(hipMemcpy(out_ids, d_out_ids.p, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToHost));
    PCV_HIP(hipMemcpy(out_neighbor_ids, d_out_nbr.p, (size_t)rows * k * sizeof(int64_t), hipMemcpyDeviceToHost));
    PCV_HIP(hipMemcpy(out_scores, d_out_score.p, (size_t)rows * k * sizeof(float), hipMemcpyDeviceToHost));
    PCV_HIP(hipMemcpy(out_counts, d_out_count.p, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (groups && out_groups) PCV_HIP(hipMemcpy(out_groups, d_out_grp.p, (size_t)rows * k * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (groups) rg.finish(job, s->pair_group_stats);
    int64_t listed = 0;
    for (int64_t i = 0; i < rows; ++i) listed += out_counts[i];
    stats.listed = listed;
}

// ---- item matches (pcv_searcher_match; DESIGN.md §4 "Item matches") ----
// The neighbours' steps over a rectangle: owners from one selection of segments, partners from another.  The launch is ordered
// [to only | to and from | from only], each part in position order: the partners are then the block prefix every wave streams, the
// owners the block suffix the tiles are cut from, and the work is |from| x |to| whatever the two selections share.  The launch order
// is not the position order any more: seg_out0 carries each `from` segment's place in the outputs, and the select step breaks ties
// by the order rows of the job (fill_position_order).  Everything the call allocates is its own and is given back when it ends.
// `groups` (match_grouped): as for the neighbours.
void match(pcv_searcher* s, const int64_t* from_source_ids, int n_from, const int64_t* to_source_ids, int n_to, int k, float min_score,
           int64_t capacity, int64_t* out_ids, int64_t* out_match_ids, float* out_scores, int32_t* out_counts, int64_t* out_rows,
           const pcv_searcher* groups = nullptr, uint32_t flags = 0, int64_t* out_groups = nullptr) {
    PCV_REQUIRE(!s->dirty, "match: rows were added or cleared without pcv_searcher_finalize");
    PCV_REQUIRE(s->shard_offset == 0, "match: a sharded searcher (set_shard_offset) is not supported");
    const std::vector<SelSeg> from = select_segments(s, from_source_ids, n_from);
    const int64_t n = selected_rows(from);
    *out_rows = n;
    if (out_ids == nullptr && capacity == 0) return;  // the count alone
    PCV_REQUIRE(capacity >= n, "match: the outputs have room for %lld rows, the selected sources have %lld", (long long)capacity, (long long)n);
    s->match_stats = pcv_match_stats{};
    if (groups) s->pair_group_stats = pcv_pair_group_stats{};
    const int tile = mfma_pass_queries(s->Dp);
    if (tile == 0) PCV_FAIL(PCV_ERR_UNSUPPORTED, "match: a bf16 tile of %d-d rows does not fit the LDS", s->D);
    if (groups) {
        s->pair_group_stats.flags = flags;
        s->pair_group_stats.bound_tile_rows = flags != 0 ? std::min(tile, 2 * (int)kBlockRows) : tile;
    }
    if (n == 0) return;
    const std::vector<SelSeg> to = select_segments(s, to_source_ids, n_to);
    auto among = [](const std::vector<SelSeg>& v, const Segment* g) {
        return std::any_of(v.begin(), v.end(), [&](const SelSeg& x) { return x.g == g; });
    };
    // the launch order and, beside it, the output index of each segment's row 0 (-1: no owners in it)
    std::vector<SelSeg> segs;
    std::vector<int64_t> out0;
    uint32_t owner_block0 = 0, partner_blocks = 0;
    for (const SelSeg& g : to)
        if (!among(from, g.g)) {
            segs.push_back(g);
            out0.push_back(-1);
            owner_block0 += g.g->nblocks();
        }
    partner_blocks = owner_block0;
    for (int both = 1; both >= 0; --both) {
        int64_t o = 0;
        for (const SelSeg& g : from) {
            if ((int)among(to, g.g) == both) {
                segs.push_back(g);
                out0.push_back(o);
                if (both) partner_blocks += g.g->nblocks();
            }
            o += g.g->nrows;
        }
    }
    NeighborPlan plan;
    RowGroups rg;
    DevBuf<float> d_out_score;
    DevBuf<unsigned long long> d_cnt;
    DevBuf<int64_t> d_out_ids, d_out_nbr, d_out_grp;
    DevBuf<int32_t> d_out_count;
    RowsJob job(s, segs, "match", PCV_METRIC_COSINE, (uint32_t)tile / kBlockRows, out0.data());
    hipStream_t st = job.st;
    const ScanParams& p = *job.p;
    const ScanParams* dp = job.dp;

    d_cnt.ensure(1);
    if (groups) {
        rg.open(job, groups);
        plan.with_groups(rg, flags);
        d_out_grp.ensure((size_t)n * k);
        plan.a.out_grp = d_out_grp.p;
    }
    plan.open_ranges(job, (uint32_t)tile / kBlockRows, k, selfjoin_margin(s->Dp), d_cnt.p, owner_block0, partner_blocks, min_score, n);
    NeighborArgs& a = plan.a;
    d_out_ids.ensure((size_t)n);
    d_out_nbr.ensure((size_t)n * k);
    d_out_score.ensure((size_t)n * k);
    d_out_count.ensure((size_t)n);
    a.out_ids = d_out_ids.p;
    a.out_nbr = d_out_nbr.p;
    a.out_score = d_out_score.p;
    a.out_count = d_out_count.p;

    pcv_match_stats& stats = s->match_stats;
    stats.rows = n;
    stats.partner_rows = selected_rows(to);
    stats.owner_blocks = (int32_t)(p.total_blocks - owner_block0);
    stats.partner_blocks = (int32_t)partner_blocks;
    stats.k = k;
    stats.tile_rows = tile;
    stats.sample_stride = (int32_t)a.stride;
    stats.spans = (int32_t)a.spans;

    unsigned long long count[1] = {0}, again[1] = {0};
    plan.zero(st);
    PCV_HIP(hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned long long), st));
    if (groups) rg.zero(st);
    job.prep();
    if (groups) {  // (as in `neighbors`)
        rg.gather(job);
        job.record(1);
    }
    const Listing list = plan.list(job, count, again);
    stats.prep_ms = job.elapsed(0) - (groups ? job.elapsed(6) : 0.0f);
    stats.bound_ms = job.elapsed(1);
    stats.screen_ms = list.ms;
    const uint64_t n_cand = count[0];
    stats.candidates = (int64_t)n_cand;
    if (n_cand > kMaxNeighborCandidates)
        PCV_FAIL(PCV_ERR_UNSUPPORTED,
                 "match: the list pass leaves %llu candidates for k = %d and min_score %g, more than %llu: ask for fewer matches, a higher bound or "
                 "fewer rows",
                 (unsigned long long)n_cand, k, (double)min_score, (unsigned long long)kMaxNeighborCandidates);
    if (list.repeated) {  // (the pass lists the same pairs again)
        PCV_REQUIRE(again[0] == n_cand, "match: the repeated list pass left %llu candidates, the first %llu", again[0], (unsigned long long)n_cand);
        stats.reruns = 1;
        stats.screen_ms += list.again_ms;
    }
    plan.rescore(job, n_cand);
    job.record(4);
    launch_neighbors_select(st, p, dp, a);
    job.record(5);
    job.wait();
    stats.rescore_ms = job.elapsed(3);
    stats.select_ms = job.elapsed(4);
    PCV_HIP(hipMemcpy(out_ids, d_out_ids.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    PCV_HIP(hipMemcpy(out_match_ids, d_out_nbr.p, (size_t)n * k * sizeof(int64_t), hipMemcpyDeviceToHost));
    PCV_HIP(hipMemcpy(out_scores, d_out_score.p, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost));
    PCV_HIP(hipMemcpy(out_counts, d_out_count.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (groups && out_groups) PCV_HIP(hipMemcpy(out_groups, d_out_grp.p, (size_t)n * k * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (groups) rg.finish(job, s->pair_group_stats);
    int64_t listed = 0;
    for (int64_t i = 0; i < n; ++i) listed += out_counts[i];
    stats.listed = listed;
}

// ---- density clusters (pcv_searcher_density_clusters; DESIGN.md §4 "Density clusters") ----
constexpr uint64_t kMaxDensityBand = (uint64_t)1 << 28;  // band pairs the degree pass may list: 8 bytes each, and 8 more if confirmed
constexpr int64_t kMaxDensityRows = (int64_t)1 << 30;

// Prep, degree pass, rescore of the band, core flags, link pass, labels (density_kernels.hip), with find_duplicates' plumbing: the
// row table, the tile choice, the spans and the rerun-once rule for a short band list.  The host waits where the band count decides
// an allocation and at the end.  Everything the call allocates is its own and is given back when it ends: nothing of the searcher's
// pass state is touched, and only the f32 rows are read.
void density_clusters(pcv_searcher* s, const int64_t* source_ids, int n_sources, float threshold, int min_items, int64_t capacity,
                      int64_t* out_ids, int32_t* out_label, int8_t* out_kind, int32_t* out_degree, int64_t* out_rows, int32_t* out_clusters) {
    PCV_REQUIRE(!s->dirty, "density_clusters: rows were added or cleared without pcv_searcher_finalize");
    PCV_REQUIRE(s->shard_offset == 0, "density_clusters: a sharded searcher (set_shard_offset) is not supported");
    const std::vector<SelSeg> segs = select_segments(s, source_ids, n_sources);
    const int64_t n = selected_rows(segs);
    *out_rows = n;
    s->density_stats = pcv_density_stats{};
    if (out_label == nullptr && capacity == 0) return;  // the count alone
    PCV_REQUIRE(capacity >= n, "density_clusters: the outputs have room for %lld rows, the selected sources have %lld", (long long)capacity,
                (long long)n);
    const int tile = mfma_pass_queries(s->Dp);
    if (tile == 0) PCV_FAIL(PCV_ERR_UNSUPPORTED, "density_clusters: a bf16 tile of %d-d rows does not fit the LDS", s->D);
    if (n > kMaxDensityRows) PCV_FAIL(PCV_ERR_UNSUPPORTED, "density_clusters: %lld rows, more than 2^30", (long long)n);
    *out_clusters = 0;
    if (n == 0) return;
    DevBuf<unsigned long long> d_cnt;
    DevBuf<uint64_t> d_cand, d_conf;
    DevBuf<uint32_t> d_degree, d_rows4;  // d_rows4: parent, attach, root, rank
    DevBuf<uint8_t> d_core;
    DevBuf<int32_t> d_label, d_out_degree;
    DevBuf<int8_t> d_kind;
    DevBuf<int64_t> d_out_ids;
    DensityArgs a{};
    a.tile_blocks = (uint32_t)tile / kBlockRows;
    RowsJob job(s, segs, "density_clusters", PCV_METRIC_COSINE, a.tile_blocks);
    hipStream_t st = job.st;
    const ScanParams& p = *job.p;
    const ScanParams* dp = job.dp;
    const int64_t rows = job.rows;

    a.span_blocks = kJoinSpanBlocks;
    while ((p.total_blocks + a.span_blocks - 1) / a.span_blocks > 65535u) a.span_blocks *= 2;  // (the grid's second dimension)
    // thr + margin rounded up, thr - margin rounded down, both from f64: s >= hi certifies c >= thr, s < lo certifies c < thr
    const double margin = (double)selfjoin_margin(s->Dp);
    a.threshold = (double)threshold;
    a.hi = std::nextafterf((float)((double)threshold + margin), INFINITY);
    a.lo = std::nextafterf((float)((double)threshold - margin), -INFINITY);
    a.min_items = min_items;
    const size_t nr = job.nr, n_pad = job.n_rinv;
    d_cnt.ensure(kDensityCounters);
    d_degree.ensure(n_pad);
    d_core.ensure(n_pad);
    d_rows4.ensure(4 * nr);
    d_label.ensure((size_t)rows);
    d_out_degree.ensure((size_t)rows);
    d_kind.ensure((size_t)rows);
    d_out_ids.ensure((size_t)rows);
    a.cand_cap = std::min<uint64_t>(kMaxDensityBand, std::max<uint64_t>(65536, 2 * (uint64_t)rows));
    d_cand.ensure(a.cand_cap);
    a.rinv = job.d_rinv.p;
    a.norm = job.d_norm.p;
    a.counters = d_cnt.p;
    a.degree = d_degree.p;
    a.core = d_core.p;
    a.parent = d_rows4.p;
    a.attach = d_rows4.p + nr;
    a.root = d_rows4.p + 2 * nr;
    a.rank = d_rows4.p + 3 * nr;
    a.seg_out0 = job.seg_out0;
    a.out_label = d_label.p;
    a.out_kind = d_kind.p;
    a.out_degree = d_out_degree.p;
    a.out_ids = d_out_ids.p;

    pcv_density_stats& stats = s->density_stats;
    stats.rows = rows;
    stats.tile_rows = tile;

    unsigned long long counts[kDensityCounters] = {}, again[kDensityCounters] = {};
    PCV_HIP(hipMemsetAsync(d_degree.p, 0, n_pad * sizeof(uint32_t), st));
    PCV_HIP(hipMemsetAsync(d_core.p, 0, n_pad * sizeof(uint8_t), st));
    PCV_HIP(hipMemsetAsync(d_cnt.p, 0, kDensityCounters * sizeof(unsigned long long), st));
    job.prep();
    static_assert(kDensityBand == 0, "the band count is the counter the listing rule reads");
    const Listing degree = list_candidates(
        job, 1, d_cnt.p, counts, again, a.cand_cap, kMaxDensityBand,
        [&] {
            a.cand = d_cand.p;
            launch_density_degree(st, p, dp, a);
        },
        [&] {  // (the pass adds to the degrees and to the sure pairs as well)
            PCV_HIP(hipMemsetAsync(d_degree.p, 0, n_pad * sizeof(uint32_t), st));
            PCV_HIP(hipMemsetAsync(d_cnt.p, 0, kDensityCounters * sizeof(unsigned long long), st));
        },
        d_cand);
    stats.prep_ms = job.elapsed(0);
    stats.degree_ms = degree.ms;
    const uint64_t n_cand = counts[kDensityBand];
    stats.candidates = (int64_t)n_cand;
    stats.sure_pairs = (int64_t)counts[kDensitySure];
    if (n_cand > kMaxDensityBand)
        PCV_FAIL(PCV_ERR_UNSUPPORTED,
                 "density_clusters: %llu pairs lie within the screen's margin of threshold %g or hold a row it is not certified for, more than "
                 "%llu (2^28): move the threshold or cluster fewer rows",
                 (unsigned long long)n_cand, (double)threshold, (unsigned long long)kMaxDensityBand);
    if (degree.repeated) {  // (the pass finds the same pairs again)
        PCV_REQUIRE(again[kDensityBand] == n_cand && again[kDensitySure] == (unsigned long long)stats.sure_pairs,
                    "density_clusters: the repeated degree pass found %llu band and %llu sure pairs, the first %llu and %lld", again[kDensityBand],
                    again[kDensitySure], (unsigned long long)n_cand, (long long)stats.sure_pairs);
        stats.reruns = 1;
        stats.degree_ms += degree.again_ms;
    }
    a.n_cand = n_cand;
    d_conf.ensure((size_t)std::max<uint64_t>(1, n_cand));
    a.conf = d_conf.p;
    job.record(2);
    launch_density_rescore(st, p, dp, a);
    job.record(3);
    launch_density_core(st, p, a);
    launch_density_link(st, p, dp, a);
    job.record(4);
    launch_density_labels(st, p, dp, a);
    job.record(5);
    PCV_HIP(hipMemcpyAsync(counts, d_cnt.p, sizeof(counts), hipMemcpyDeviceToHost, st));
    job.wait();
    stats.rescore_ms = job.elapsed(2);
    stats.link_ms = job.elapsed(3);
    stats.label_ms = job.elapsed(4);
    stats.confirmed = (int64_t)counts[kDensityConfirmed];
    stats.participating = (int64_t)counts[kDensityParticipating];
    stats.core = (int64_t)counts[kDensityCore];
    stats.border = (int64_t)counts[kDensityBorder];
    stats.noise = (int64_t)counts[kDensityNoise];
    stats.clusters = (int32_t)counts[kDensityClusters];
    PCV_HIP(hipMemcpy(out_label, d_label.p, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    PCV_HIP(hipMemcpy(out_kind, d_kind.p, (size_t)rows * sizeof(int8_t), hipMemcpyDeviceToHost));
    if (out_degree) PCV_HIP(hipMemcpy(out_degree, d_out_degree.p, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_ids) PCV_HIP(hipMemcpy(out_ids, d_out_ids.p, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToHost));
    *out_clusters = stats.clusters;
}

// ---- linkage tree and reach tree (pcv_searcher_linkage_tree, pcv_searcher_reach_tree; DESIGN.md §4 "Linkage tree", "Reach tree") ----
constexpr uint64_t kMaxLinkageCandidates = (uint64_t)1 << 28;  // directed pairs one round's list pass may leave: 16 bytes each
constexpr int64_t kMaxLinkageRows = (int64_t)1 << 30;

// The Borůvka rounds of both trees (linkage_kernels.hip): bound pass, thresholds, list pass, rescore and choice, merge, with the
// neighbours' plumbing — the row table, the tile choice, the sampled bound pass and the rerun-once rule for a short list.  The host
// waits where a count decides an allocation and at the end of a round, where it checks that the round emitted one edge per component
// it removed and at least halved their number: no loop here can run on without progress.  The trees differ in three launches of a
// round (bound, list, rescore), which `run` takes as callables, and in their stats structs, whose shared fields `Stats` names.
// Declared before the call's RowsJob, as every buffer is.
struct LinkRounds {
    DevBuf<unsigned long long> d_cnt, d_cand_key, d_best, d_edges;  // d_best: best_key, best_pair;  d_edges: edge_pair, edge_key
    DevBuf<uint64_t> d_cand;
    DevBuf<uint32_t> d_comp, d_rows3;  // d_rows3: parent, cert, comp_max
    DevBuf<float> d_thr;
    DevBuf<int64_t> d_out_ids;
    DevBuf<int8_t> d_out_part;
    uint32_t sample_stride = 1;
    size_t nr = 0, n_pad = 0;
    uint64_t P = 0, emitted = 0;  // participating rows; edges
    unsigned long long counts[kLinkCounters] = {}, again[kLinkCounters] = {};

    // The buffers every round uses and their wiring into `a` (whose tile_blocks the caller has set), the zeroing — `zero_more` queues
    // the caller's own between comp's and the counters', of which the caller may keep `more_counters` of its own behind kLinkCounters
    // — prep, begin and the participating count.
    template <class Stats, class Zero>
    void open(RowsJob& job, const char* what, LinkageArgs& a, int Dp, int more_counters, Stats& stats, Zero zero_more) {
        hipStream_t st = job.st;
        // The sample of the bound pass (DESIGN.md §4 "Linkage tree"): no result depends on it, only the list's length.
        const uint32_t TB = job.p->total_blocks;
        sample_stride = std::min<uint32_t>(4, std::max<uint32_t>(1, TB / 64));
        a.margin = selfjoin_margin(Dp);
        a.walk_len = walk_blocks(TB);

        nr = job.nr;
        n_pad = job.n_rinv;
        d_cnt.ensure(kLinkCounters + more_counters);
        d_comp.ensure(n_pad);
        d_rows3.ensure(3 * nr);
        d_thr.ensure(nr);
        d_best.ensure(2 * nr);
        d_edges.ensure(2 * nr);
        d_out_ids.ensure((size_t)job.rows);
        d_out_part.ensure((size_t)job.rows);
        a.rinv = job.d_rinv.p;
        a.norm = job.d_norm.p;
        a.comp = d_comp.p;
        a.parent = d_rows3.p;
        a.cert = d_rows3.p + nr;
        a.comp_max = d_rows3.p + 2 * nr;
        a.thr = d_thr.p;
        a.best_key = d_best.p;
        a.best_pair = d_best.p + nr;
        a.edge_pair = d_edges.p;
        a.edge_key = d_edges.p + nr;
        a.edge_cap = nr;
        a.counters = d_cnt.p;
        a.seg_out0 = job.seg_out0;
        a.out_ids = d_out_ids.p;
        a.out_part = d_out_part.p;

        PCV_HIP(hipMemsetAsync(d_comp.p, 0, n_pad * sizeof(uint32_t), st));
        zero_more();
        PCV_HIP(hipMemsetAsync(d_cnt.p, 0, (kLinkCounters + more_counters) * sizeof(unsigned long long), st));
        job.prep();
        launch_linkage_begin(st, *job.p, a);
        PCV_HIP(hipMemcpyAsync(counts, d_cnt.p, sizeof(counts), hipMemcpyDeviceToHost, st));
        job.wait();
        stats.prep_ms = job.elapsed(0);
        P = counts[kLinkParticipating];
        stats.participating = (int64_t)P;
        PCV_REQUIRE(P <= (uint64_t)job.rows, "%s: %llu participating rows of %lld", what, (unsigned long long)P, (long long)job.rows);
    }

    // The candidate buffers (allocated here, behind whatever the caller gave back since `open`), the rounds until one component is
    // left, and the edge count.  `same`: what the rows of a list that grew too long are nearly the same of ("distance", "reach").
    template <class Stats, class Bound, class List, class Rescore>
    void run(RowsJob& job, const char* what, const char* same, LinkageArgs& a, Stats& stats, Bound bound, List list_pass, Rescore rescore) {
        hipStream_t st = job.st;
        const ScanParams& p = *job.p;
        a.cand_cap = std::min<uint64_t>(kMaxLinkageCandidates, std::max<uint64_t>(65536, (uint64_t)32 * (uint64_t)nr));
        d_cand.ensure(a.cand_cap);
        d_cand_key.ensure(a.cand_cap);

        // PCV_LINKAGE_ROUNDS_FILE (tools/bench_linkage.py, tools/bench_reach.py): one line per round is appended to that file — round,
        // components before and after, candidates, bound repeated at stride 1 (0 / 1), list reruns, and the round's bound, list,
        // rescore and merge ms
        FILE* round_log = nullptr;
        if (const char* f = getenv("PCV_LINKAGE_ROUNDS_FILE")) round_log = std::fopen(f, "a");
        struct CloseLog {
            FILE* f;
            ~CloseLog() {
                if (f) std::fclose(f);
            }
        } close_log{round_log};

        uint64_t components = P;
        emitted = 0;
        while (components > 1) {
            bool bound_repeated = false;
            // 1. the bound of every component, and its threshold
            auto queue_bound = [&](uint32_t stride) {
                PCV_HIP(hipMemsetAsync(d_cnt.p + kLinkUnbounded, 0, 2 * sizeof(unsigned long long), st));
                static_assert(kLinkCertRoots == kLinkUnbounded + 1, "the two counters of the threshold step are reset together");
                a.stride = stride;
                bound();
                launch_linkage_threshold(st, p, a);
            };
            PCV_HIP(hipMemsetAsync(d_rows3.p + nr, 0, 2 * nr * sizeof(uint32_t), st));  // cert, comp_max
            PCV_HIP(hipMemsetAsync(d_best.p, 0, nr * sizeof(unsigned long long), st));
            PCV_HIP(hipMemsetAsync(d_best.p + nr, 0xff, nr * sizeof(unsigned long long), st));
            PCV_HIP(hipMemsetAsync(d_cnt.p + kLinkListed, 0, sizeof(unsigned long long), st));
            PCV_HIP(hipMemsetAsync(d_cnt.p + kLinkRoots, 0, sizeof(unsigned long long), st));
            job.record(0);
            queue_bound(sample_stride);
            if (sample_stride > 1) {
                // a component with a certified row that met no certified foreign row in the sample, while there is one somewhere:
                // without a bound it would list every foreign partner of every row it has.  Once more over every block (max commutes:
                // what the sample found stays).
                PCV_HIP(hipMemcpyAsync(counts, d_cnt.p, sizeof(counts), hipMemcpyDeviceToHost, st));
                job.wait();
                bound_repeated = counts[kLinkUnbounded] > 0 && counts[kLinkCertRoots] >= 2;
                if (bound_repeated) queue_bound(1);
            }
            job.record(1);
            // 2. the candidates
            a.stride = 1;
            const Listing list = list_candidates(
                job, 1, d_cnt.p, counts, again, a.cand_cap, kMaxLinkageCandidates,
                [&] {
                    a.cand = d_cand.p;
                    a.cand_key = d_cand_key.p;
                    list_pass();
                },
                [&] { PCV_HIP(hipMemsetAsync(d_cnt.p + kLinkListed, 0, sizeof(unsigned long long), st)); }, d_cand, d_cand_key);
            static_assert(kLinkListed == 0, "the listed count is the counter the listing rule reads");
            const float round_bound_ms = job.elapsed(0), round_list_ms = list.ms + (list.repeated ? list.again_ms : 0.0f);
            stats.bound_ms += round_bound_ms;
            stats.list_ms += list.ms;
            const uint64_t n_cand = counts[kLinkListed];
            if (n_cand > kMaxLinkageCandidates)
                PCV_FAIL(PCV_ERR_UNSUPPORTED,
                         "%s: round %d lists %llu candidate pairs, more than %llu (2^28): too many rows are nearly the same %s from their "
                         "nearest foreign row, or lie outside the lengths the screen is certified for; build the tree of fewer rows",
                         what, (int)stats.rounds, (unsigned long long)n_cand, (unsigned long long)kMaxLinkageCandidates, same);
            if (list.repeated) {  // (the pass lists the same pairs again)
                PCV_REQUIRE(again[kLinkListed] == n_cand, "%s: the repeated list pass left %llu candidates, the first %llu", what, again[kLinkListed],
                            (unsigned long long)n_cand);
                stats.reruns += 1;
                stats.list_ms += list.again_ms;
            }
            stats.candidates += (int64_t)n_cand;
            stats.rounds += 1;
            // 3. the f64 decision, 4. the merge
            a.n_cand = n_cand;
            job.record(3);
            rescore();
            job.record(4);
            launch_linkage_merge(st, p, a);
            job.record(5);
            PCV_HIP(hipMemcpyAsync(counts, d_cnt.p, sizeof(counts), hipMemcpyDeviceToHost, st));
            job.wait();
            stats.rescore_ms += job.elapsed(3);
            stats.merge_ms += job.elapsed(4);
            // 5. one edge per component that went, and at least every second one went
            const uint64_t after = counts[kLinkRoots], now = counts[kLinkEmitted];
            if (!(after >= 1 && after <= components / 2 && now - emitted == components - after))
                PCV_FAIL(PCV_ERR_INTERNAL, "%s: round %d went from %llu components to %llu and emitted %llu edges", what, (int)stats.rounds - 1,
                         (unsigned long long)components, (unsigned long long)after, (unsigned long long)(now - emitted));
            if (round_log)
                std::fprintf(round_log, "%d %llu %llu %llu %d %d %.4f %.4f %.4f %.4f\n", (int)stats.rounds - 1, (unsigned long long)components,
                             (unsigned long long)after, (unsigned long long)n_cand, bound_repeated ? 1 : 0, list.repeated ? 1 : 0, round_bound_ms,
                             round_list_ms, job.elapsed(3), job.elapsed(4));
            components = after;
            emitted = now;
        }
        PCV_REQUIRE(emitted == (P > 0 ? P - 1 : 0), "%s: %llu edges for %llu participating rows", what, (unsigned long long)emitted, (unsigned long long)P);
        stats.edges = (int64_t)emitted;
        a.n_edges = emitted;
    }
};

// What both trees check before they open a job.  -> the rows of the LDS tile; 0: the count alone was asked for, or there are no rows
int tree_arguments(pcv_searcher* s, const char* what, int64_t n, const int64_t* out_pos_a, int64_t capacity, int64_t* out_edges) {
    if (out_pos_a == nullptr && capacity == 0) return 0;  // the count alone
    PCV_REQUIRE(capacity >= n, "%s: the outputs have room for %lld rows, the selected sources have %lld", what, (long long)capacity, (long long)n);
    const int tile = mfma_pass_queries(s->Dp);
    if (tile == 0) PCV_FAIL(PCV_ERR_UNSUPPORTED, "%s: a bf16 tile of %d-d rows does not fit the LDS", what, s->D);
    if (n > kMaxLinkageRows) PCV_FAIL(PCV_ERR_UNSUPPORTED, "%s: %lld rows, more than 2^30", what, (long long)n);
    *out_edges = 0;
    return n == 0 ? 0 : tile;
}

// The n edges the output step left in `d`, in the order the trees return them: key descending (c or w), then the two positions
// ascending; the columns every tree has are written here.
template <class Edge, class Key>
std::vector<Edge> edges_in_order(const DevBuf<Edge>& d, uint64_t n, Key key, int64_t* out_pos_a, int64_t* out_pos_b, double* out_key, int64_t* out_id_a,
                                 int64_t* out_id_b) {
    std::vector<Edge> edges((size_t)n);
    if (n > 0) PCV_HIP(hipMemcpy(edges.data(), d.p, (size_t)n * sizeof(Edge), hipMemcpyDeviceToHost));
    std::sort(edges.begin(), edges.end(), [&](const Edge& x, const Edge& y) {
        if (key(x) != key(y)) return key(x) > key(y);
        if (x.pos_a != y.pos_a) return x.pos_a < y.pos_a;
        return x.pos_b < y.pos_b;
    });
    for (size_t i = 0; i < edges.size(); ++i) {
        out_pos_a[i] = edges[i].pos_a;
        out_pos_b[i] = edges[i].pos_b;
        out_key[i] = key(edges[i]);
        if (out_id_a) {
            out_id_a[i] = edges[i].id_a;
            out_id_b[i] = edges[i].id_b;
        }
    }
    return edges;
}

// Prep, the rounds of LinkRounds with the linkage screen, the outputs.  Everything the call allocates is its own and is given back
// when it ends: nothing of the searcher's pass state is touched, and only the f32 rows are read.
void linkage_tree(pcv_searcher* s, const int64_t* source_ids, int n_sources, int64_t capacity, int64_t* out_ids, int8_t* out_part, int64_t* out_pos_a,
                  int64_t* out_pos_b, int64_t* out_id_a, int64_t* out_id_b, double* out_c, int64_t* out_rows, int64_t* out_edges) {
    PCV_REQUIRE(!s->dirty, "linkage_tree: rows were added or cleared without pcv_searcher_finalize");
    PCV_REQUIRE(s->shard_offset == 0, "linkage_tree: a sharded searcher (set_shard_offset) is not supported");
    const std::vector<SelSeg> segs = select_segments(s, source_ids, n_sources);
    const int64_t n = selected_rows(segs);
    *out_rows = n;
    s->linkage_stats = pcv_linkage_stats{};
    const int tile = tree_arguments(s, "linkage_tree", n, out_pos_a, capacity, out_edges);
    if (tile == 0) return;
    LinkRounds rounds;
    DevBuf<LinkEdge> d_out_edges;
    LinkageArgs a{};
    a.tile_blocks = (uint32_t)tile / kBlockRows;
    RowsJob job(s, segs, "linkage_tree", PCV_METRIC_COSINE, a.tile_blocks);
    hipStream_t st = job.st;
    const ScanParams& p = *job.p;
    const ScanParams* dp = job.dp;
    const int64_t rows = job.rows;

    pcv_linkage_stats& stats = s->linkage_stats;
    stats.rows = rows;
    stats.tile_rows = tile;
    rounds.open(job, "linkage_tree", a, s->Dp, 0, stats, [] {});
    rounds.run(
        job, "linkage_tree", "distance", a, stats, [&] { launch_linkage_bound(st, p, dp, a); }, [&] { launch_linkage_list(st, p, dp, a); },
        [&] { launch_linkage_rescore(st, p, dp, a); });

    const uint64_t emitted = rounds.emitted;
    d_out_edges.ensure((size_t)std::max<uint64_t>(1, emitted));
    a.out_edges = d_out_edges.p;
    launch_linkage_output(st, p, dp, a);
    job.wait();
    edges_in_order(d_out_edges, emitted, [](const LinkEdge& e) { return e.c; }, out_pos_a, out_pos_b, out_c, out_id_a, out_id_b);
    if (out_ids) PCV_HIP(hipMemcpy(out_ids, rounds.d_out_ids.p, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (out_part) PCV_HIP(hipMemcpy(out_part, rounds.d_out_part.p, (size_t)rows * sizeof(int8_t), hipMemcpyDeviceToHost));
    *out_edges = (int64_t)emitted;
}

// Prep, the core step — the neighbours' bound, thresholds, list and rescore with k = j (NeighborPlan), then the j-th best f64 c of
// every row and its two f32 images (reach_kernels.hip) — and the rounds of LinkRounds with the capped screen and the capped weight.
// The core step's buffers go back before the rounds allocate their candidate lists.  Nothing of the searcher's pass state is touched,
// and only the f32 rows are read.
void reach_tree(pcv_searcher* s, const int64_t* source_ids, int n_sources, int min_items, int64_t capacity, int64_t* out_ids, int8_t* out_part,
                double* out_core, int64_t* out_pos_a, int64_t* out_pos_b, int64_t* out_id_a, int64_t* out_id_b, double* out_w, double* out_c,
                int64_t* out_rows, int64_t* out_edges) {
    PCV_REQUIRE(!s->dirty, "reach_tree: rows were added or cleared without pcv_searcher_finalize");
    PCV_REQUIRE(s->shard_offset == 0, "reach_tree: a sharded searcher (set_shard_offset) is not supported");
    const std::vector<SelSeg> segs = select_segments(s, source_ids, n_sources);
    const int64_t n = selected_rows(segs);
    *out_rows = n;
    s->reach_stats = pcv_reach_stats{};
    const int tile = tree_arguments(s, "reach_tree", n, out_pos_a, capacity, out_edges);
    if (tile == 0) return;
    LinkRounds rounds;
    NeighborPlan core;
    DevBuf<float> d_k2;  // klo, khi
    DevBuf<double> d_core, d_out_core;
    DevBuf<ReachEdge> d_out_edges;
    ReachArgs ra{};
    LinkageArgs& a = ra.l;
    a.tile_blocks = (uint32_t)tile / kBlockRows;
    RowsJob job(s, segs, "reach_tree", PCV_METRIC_COSINE, a.tile_blocks);
    hipStream_t st = job.st;
    const ScanParams& p = *job.p;
    const ScanParams* dp = job.dp;
    const int64_t rows = job.rows;

    const size_t nr = job.nr, n_pad = job.n_rinv;
    constexpr int kReachListed = kLinkCounters, kReachShort = kLinkCounters + 1;  // the core step's two counters, behind the rounds'
    d_k2.ensure(2 * n_pad);
    d_core.ensure(nr);
    d_out_core.ensure((size_t)rows);
    ra.core = d_core.p;
    ra.klo = d_k2.p;
    ra.khi = d_k2.p + n_pad;
    ra.out_core = d_out_core.p;

    pcv_reach_stats& stats = s->reach_stats;
    stats.rows = rows;
    stats.tile_rows = tile;
    stats.min_items = min_items;
    rounds.open(job, "reach_tree", a, s->Dp, 2, stats, [&] { PCV_HIP(hipMemsetAsync(d_k2.p, 0, 2 * n_pad * sizeof(float), st)); });
    ra.short_rows = a.counters + kReachShort;
    const uint64_t P = rounds.P;

    // The core step.  j = 0: every core is +inf and the neighbours have nothing to say.
    const int j = (int)std::min<uint64_t>((uint64_t)(min_items - 1), P > 0 ? P - 1 : 0);
    ra.k = j;
    if (j >= 1) {
        core.open(job, a.tile_blocks, j, a.margin, a.counters + kReachListed);
        core.zero(st);
        job.record(1);
        unsigned long long listed[1] = {0}, listed_again[1] = {0};
        const Listing list = core.list(job, listed, listed_again);
        stats.core_ms = job.elapsed(1) + list.ms;
        const uint64_t n_core = listed[0];
        stats.core_candidates = (int64_t)n_core;
        if (n_core > kMaxNeighborCandidates)
            PCV_FAIL(PCV_ERR_UNSUPPORTED,
                     "reach_tree: the core step lists %llu candidate pairs for min_items = %d, more than %llu (2^30): ask for fewer items or fewer rows",
                     (unsigned long long)n_core, min_items, (unsigned long long)kMaxNeighborCandidates);
        if (list.repeated) {
            PCV_REQUIRE(listed_again[0] == n_core, "reach_tree: the repeated list pass of the core step left %llu candidates, the first %llu", listed_again[0],
                        (unsigned long long)n_core);
            stats.reruns += 1;
            stats.core_ms += list.again_ms;
        }
        core.rescore(job, n_core);
        ra.row_off = core.a.row_off;
        ra.sorted_key = core.a.sorted_key;
        launch_reach_core(st, p, ra);
        job.record(4);
        unsigned long long short_rows = 0;
        PCV_HIP(hipMemcpyAsync(&short_rows, ra.short_rows, sizeof(short_rows), hipMemcpyDeviceToHost, st));
        job.wait();
        stats.core_ms += job.elapsed(3);
        if (short_rows != 0)
            PCV_FAIL(PCV_ERR_INTERNAL, "reach_tree: %llu participating rows were left fewer than %d rescored partners", short_rows, j);
        core.release();
    } else {
        launch_reach_core(st, p, ra);
    }
    rounds.run(
        job, "reach_tree", "reach", a, stats, [&] { launch_linkage_bound(st, p, dp, a, ra.klo); }, [&] { launch_linkage_list(st, p, dp, a, ra.khi); },
        [&] { launch_reach_rescore(st, p, dp, ra); });

    const uint64_t emitted = rounds.emitted;
    d_out_edges.ensure((size_t)std::max<uint64_t>(1, emitted));
    ra.out_edges = d_out_edges.p;
    launch_reach_output(st, p, dp, ra);
    job.wait();
    const std::vector<ReachEdge> edges =
        edges_in_order(d_out_edges, emitted, [](const ReachEdge& e) { return e.w; }, out_pos_a, out_pos_b, out_w, out_id_a, out_id_b);
    if (out_c)
        for (size_t i = 0; i < edges.size(); ++i) out_c[i] = edges[i].c;
    if (out_ids) PCV_HIP(hipMemcpy(out_ids, rounds.d_out_ids.p, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (out_part) PCV_HIP(hipMemcpy(out_part, rounds.d_out_part.p, (size_t)rows * sizeof(int8_t), hipMemcpyDeviceToHost));
    if (out_core) PCV_HIP(hipMemcpy(out_core, d_out_core.p, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost));
    *out_edges = (int64_t)emitted;
}

// ---- seed items (pcv_searcher_seeds; DESIGN.md §4 "Seed items") ----
// Prep, begin, then k picks with a cover step between them (seed_kernels.hip): 2k launches queued on the searcher's stream and one
// wait behind the last.  Everything the call allocates is its own and is given back when it ends: nothing of the searcher's pass
// state is touched, and only the f32 rows are read.  The outputs are written last, after every check.
void seeds(pcv_searcher* s, const int64_t* source_ids, int n_sources, int k, int method, uint64_t seed, const int64_t* first_id, int64_t* out_ids,
           int64_t* out_positions, int64_t* out_totals, float* out_cover, int32_t* out_count) {
    PCV_REQUIRE(!s->dirty, "seeds: rows were added or cleared without pcv_searcher_finalize");
    PCV_REQUIRE(s->shard_offset == 0, "seeds: a sharded searcher (set_shard_offset) is not supported");
    const std::vector<SelSeg> segs = select_segments(s, source_ids, n_sources);
    s->seed_stats = pcv_seed_stats{};
    s->seed_stats.method = method;
    std::vector<int64_t> ids((size_t)k, -1), pos((size_t)k, -1), totals((size_t)k, 0);
    std::vector<float> cover((size_t)k, NAN);
    SeedState state{};
    if (!segs.empty()) {
        DevBuf<float> d_out_cover;
        DevBuf<double> d_cover;
        DevBuf<SeedPart> d_part;
        DevBuf<SeedState> d_state;
        DevBuf<int64_t> d_out;  // ids, positions, totals
        RowsJob job(s, segs, "seeds", PCV_METRIC_COSINE, 0);
        hipStream_t st = job.st;
        const ScanParams& p = *job.p;
        const ScanParams* dp = job.dp;
        s->seed_stats.rows = job.rows;

        SeedArgs a{};
        a.parts = (uint32_t)((job.nr + kSeedSpanRows - 1) / kSeedSpanRows);
        d_cover.ensure(job.nr);
        d_part.ensure(a.parts);
        d_state.ensure(1);
        d_out.ensure((size_t)3 * k);
        d_out_cover.ensure((size_t)k);
        a.rinv = job.d_rinv.p;
        a.norm = job.d_norm.p;
        a.cover = d_cover.p;
        a.part = d_part.p;
        a.state = d_state.p;
        a.out_ids = d_out.p;
        a.out_pos = d_out.p + k;
        a.out_totals = d_out.p + 2 * (size_t)k;
        a.out_cover = d_out_cover.p;
        a.method = method;
        a.seed = seed;
        a.has_first = first_id != nullptr;
        a.first_id = first_id ? *first_id : 0;

        PCV_HIP(hipMemsetAsync(d_state.p, 0, sizeof(SeedState), st));
        job.prep();
        launch_seed_begin(st, p, dp, a);
        for (int j = 0; j < k; ++j) {
            a.step = j;
            if (j > 0) launch_seed_cover(st, p, dp, a);
            launch_seed_pick(st, p, dp, a);
        }
        job.record(2);
        job.wait();
        s->seed_stats.prep_ms = job.elapsed(0);
        s->seed_stats.steps_ms = job.elapsed(1);
        PCV_HIP(hipMemcpy(&state, d_state.p, sizeof(state), hipMemcpyDeviceToHost));
        if (state.error == kSeedTooManyRows) PCV_FAIL(PCV_ERR_UNSUPPORTED, "seeds: more than 2^30 participating rows");
        if (state.error != 0 && state.error != kSeedNoFirst) PCV_FAIL(PCV_ERR_INTERNAL, "seeds: a draw outside the prefix sums (step %d)", (int)state.count);
        if (state.error == 0 && state.count > 0) {
            PCV_REQUIRE(state.count <= k, "seeds: %d picks for k = %d", (int)state.count, k);
            const size_t n = (size_t)state.count;
            PCV_HIP(hipMemcpy(ids.data(), a.out_ids, n * sizeof(int64_t), hipMemcpyDeviceToHost));
            PCV_HIP(hipMemcpy(pos.data(), a.out_pos, n * sizeof(int64_t), hipMemcpyDeviceToHost));
            PCV_HIP(hipMemcpy(totals.data(), a.out_totals, n * sizeof(int64_t), hipMemcpyDeviceToHost));
            PCV_HIP(hipMemcpy(cover.data(), a.out_cover, n * sizeof(float), hipMemcpyDeviceToHost));
        }
    }
    // (no segment selected, or no participating row: nothing carries the id either)
    if (first_id && (state.error == kSeedNoFirst || state.count == 0))
        PCV_FAIL(PCV_ERR_INVALID, "seeds: no participating row of the selected sources carries first_id %lld", (long long)*first_id);
    s->seed_stats.steps = state.count;
    s->seed_stats.participating = state.count > 0 ? totals[0] : 0;
    std::copy(ids.begin(), ids.end(), out_ids);
    std::copy(pos.begin(), pos.end(), out_positions);
    std::copy(totals.begin(), totals.end(), out_totals);
    std::copy(cover.begin(), cover.end(), out_cover);
    *out_count = state.count;
}

// ---- corpus moments and principal axes (pcv_searcher_moments, _principal_axes, _project) ----
constexpr int64_t kMaxMomentRows = (int64_t)1 << 30;  // |t| <= 2^32 (1 + 2^-23): the int64 limb sums and the 128-bit finish hold 2^30 rows
constexpr int kMaxMomentDim = 2048;

// Prep, sums, and — with a matrix asked for — the limb SYRK (moments_kernels.hip) and its 128-bit finish on the host.  The outputs
// are written last, after every check.
void moments(pcv_searcher* s, const int64_t* source_ids, int n_sources, int centered, int64_t* out_sums, double* out_matrix, int64_t* out_n) {
    PCV_REQUIRE(!s->dirty, "moments: rows were added or cleared without pcv_searcher_finalize");
    PCV_REQUIRE(s->shard_offset == 0, "moments: a sharded searcher (set_shard_offset) is not supported");
    if (s->D > kMaxMomentDim) PCV_FAIL(PCV_ERR_UNSUPPORTED, "moments: dimension %d is above %d", s->D, kMaxMomentDim);
    const std::vector<SelSeg> segs = select_segments(s, source_ids, n_sources);
    s->moment_stats = pcv_moment_stats{};
    s->moment_stats.tile_features = kMomentSide;
    const size_t D = (size_t)s->D, Dp = (size_t)s->Dp;
    std::vector<long long> S(Dp + 1, 0);
    std::vector<int64_t> hh, hl, ll;
    if (!segs.empty()) {
        DevBuf<long long> d_sums, d_mat;
        RowsJob job(s, segs, "moments", PCV_METRIC_COSINE, 0);
        job.prep();  // (it runs while the sums' room is made)
        hipStream_t st = job.st;
        s->moment_stats.rows = job.rows;
        MomentArgs a{};
        d_sums.ensure(Dp + 1);
        a.norm = job.d_norm.p;
        a.sums = d_sums.p;
        PCV_HIP(hipMemsetAsync(d_sums.p, 0, (Dp + 1) * sizeof(long long), st));
        if (out_matrix) {
            d_mat.ensure(3 * Dp * Dp);
            a.hh = d_mat.p;
            a.hl = d_mat.p + Dp * Dp;
            a.ll = d_mat.p + 2 * Dp * Dp;
            PCV_HIP(hipMemsetAsync(d_mat.p, 0, 3 * Dp * Dp * sizeof(long long), st));
            // some workgroups per CU over all the super-tiles; a chain not so short that its closing atomics show, nor above its bound
            const uint32_t TB = job.p->total_blocks, pairs = (uint32_t)((Dp / kMomentSide) * (Dp / kMomentSide));
            const uint32_t want = std::max<uint32_t>(1, 8 * (uint32_t)std::max(1, s->ctx->num_cus) / pairs);
            a.range_blocks = std::min<uint32_t>(kMomentChainBlocks, std::max<uint32_t>(8, (TB + want - 1) / want));
        }
        job.record(1);  // (behind the memsets)
        launch_moment_sums(st, *job.p, job.dp, a);
        job.record(2);
        if (out_matrix) {
            launch_moment_syrk(st, *job.p, job.dp, a);
            s->moment_stats.row_ranges = (int32_t)moment_row_ranges(*job.p, a);
        }
        job.record(3);
        PCV_HIP(hipMemcpyAsync(S.data(), d_sums.p, (Dp + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
        job.wait();
        s->moment_stats.prep_ms = job.elapsed(0);
        s->moment_stats.sums_ms = job.elapsed(1);
        s->moment_stats.syrk_ms = out_matrix ? job.elapsed(2) : 0.0f;
        s->moment_stats.participating = (int64_t)S[Dp];
        if ((int64_t)S[Dp] > kMaxMomentRows) PCV_FAIL(PCV_ERR_UNSUPPORTED, "moments: more than 2^30 participating rows");
        if (out_matrix) {  // [Dp][Dp] on the device -> [D][D]
            std::vector<long long> m(3 * Dp * Dp);
            PCV_HIP(hipMemcpy(m.data(), d_mat.p, m.size() * sizeof(long long), hipMemcpyDeviceToHost));
            hh.resize(D * D);
            hl.resize(D * D);
            ll.resize(D * D);
            for (size_t d = 0; d < D; ++d)
                for (size_t e = 0; e < D; ++e) {
                    hh[d * D + e] = (int64_t)m[d * Dp + e];
                    hl[d * D + e] = (int64_t)m[Dp * Dp + d * Dp + e];
                    ll[d * D + e] = (int64_t)m[2 * Dp * Dp + d * Dp + e];
                }
        }
    }
    std::vector<int64_t> sums(D);
    for (size_t d = 0; d < D; ++d) sums[d] = (int64_t)S[d];
    if (out_matrix) {
        if (hh.empty()) {
            std::fill(out_matrix, out_matrix + D * D, 0.0);
        } else {
            const pcv_status fin = pcv_moments_finish(hh.data(), hl.data(), ll.data(), sums.data(), (int64_t)S[Dp], s->D, centered, out_matrix);
            if (fin != PCV_OK) throw Error{fin};
        }
    }
    std::copy(sums.begin(), sums.end(), out_sums);
    *out_n = (int64_t)S[Dp];
}

void principal_axes(pcv_searcher* s, const int64_t* source_ids, int n_sources, int m, float* out_axes, double* out_offsets, double* out_variance,
                    int64_t* out_n) {
    PCV_REQUIRE(m <= s->D, "principal_axes: %d axes of a %d-d space", m, s->D);
    const size_t D = (size_t)s->D;
    std::vector<int64_t> sums(D);
    std::vector<double> cov(D * D), values(D), vectors(D * D);
    int64_t n = 0;
    moments(s, source_ids, n_sources, 1, sums.data(), cov.data(), &n);
    *out_n = n;
    PCV_REQUIRE(n > 0, "principal_axes: no participating row in the selected sources");
    const pcv_status eig = pcv_symmetric_eigen(cov.data(), s->D, values.data(), vectors.data());
    if (eig != PCV_OK) throw Error{eig};
    const double nn = (double)n;
    for (int j = 0; j < m; ++j) {
        double off = 0.0;
        for (size_t d = 0; d < D; ++d) {
            const float ax = (float)vectors[(size_t)j * D + d];
            out_axes[(size_t)j * D + d] = ax;
            const double mean = (double)sums[d] * 0x1p-32 / nn, term = (double)ax * mean;  // (no contraction: the sum is of rounded products)
            off = off + term;
        }
        out_offsets[j] = off;
        out_variance[j] = values[(size_t)j] / (nn * nn);
    }
}

// Prep, then one pass per group of axes inside project_kernel.  The axes are packed here into the rows' piece layout.
void project(pcv_searcher* s, const float* axes, const double* offsets, int m, const int64_t* source_ids, int n_sources, int64_t capacity,
             float* out_coords, int64_t* out_ids, int64_t* out_n) {
    PCV_REQUIRE(!s->dirty, "project: rows were added or cleared without pcv_searcher_finalize");
    PCV_REQUIRE(s->shard_offset == 0, "project: a sharded searcher (set_shard_offset) is not supported");
    const std::vector<SelSeg> segs = select_segments(s, source_ids, n_sources);
    const int64_t n = selected_rows(segs);
    *out_n = n;
    if (out_coords == nullptr && capacity == 0) return;  // the count alone
    PCV_REQUIRE(capacity >= n, "project: the outputs have room for %lld rows, the selected sources have %lld", (long long)capacity, (long long)n);
    s->project_stats = pcv_project_stats{};
    s->project_stats.axes = m;
    s->project_stats.group = m <= 2 ? 2 : 8;
    if (n == 0) return;
    const size_t D = (size_t)s->D, D4 = (size_t)s->D4, blocks = ((size_t)m + 31) / 32;
    std::vector<float> packed(blocks * D4 * 128, 0.0f);
    for (int j = 0; j < m; ++j) {
        float* dst = packed.data() + ((size_t)(j >> 5) * D4 * 32 + (size_t)(j & 31)) * 4;  // piece f of axis j: dst + f * 128 floats
        for (size_t d = 0; d < D; ++d) dst[(d >> 2) * 128 + (d & 3)] = axes[(size_t)j * D + d];
    }
    std::vector<double> off((size_t)m, 0.0);
    if (offsets) std::copy(offsets, offsets + m, off.begin());
    DevBuf<float> d_axes, d_coords;
    DevBuf<double> d_off;
    DevBuf<int64_t> d_ids;
    RowsJob job(s, segs, "project", PCV_METRIC_COSINE, 0);
    job.prep();  // (it runs while the outputs' room is made)
    hipStream_t st = job.st;
    s->project_stats.rows = job.rows;
    d_axes.ensure(packed.size());
    d_off.ensure((size_t)m);
    d_coords.ensure((size_t)n * m);
    if (out_ids) d_ids.ensure((size_t)n);
    ProjectArgs a{};
    a.rinv = job.d_rinv.p;
    a.norm = job.d_norm.p;
    a.axes = reinterpret_cast<const float4*>(d_axes.p);
    a.offsets = d_off.p;
    a.seg_out0 = job.seg_out0;
    a.out_coords = d_coords.p;
    a.out_ids = out_ids ? d_ids.p : nullptr;
    a.m = m;
    PCV_HIP(hipMemcpyAsync(d_axes.p, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice, st));
    PCV_HIP(hipMemcpyAsync(d_off.p, off.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
    job.record(1);  // (behind the uploads)
    launch_project(st, *job.p, job.dp, a);
    job.record(2);
    job.wait();
    s->project_stats.prep_ms = job.elapsed(0);
    s->project_stats.project_ms = job.elapsed(1);
    PCV_HIP(hipMemcpy(out_coords, d_coords.p, (size_t)n * m * sizeof(float), hipMemcpyDeviceToHost));
    if (out_ids) PCV_HIP(hipMemcpy(out_ids, d_ids.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
}

}  // namespace

extern "C" {

pcv_status pcv_searcher_find_duplicates(pcv_searcher* s, const int64_t* source_ids, int n_sources, float threshold, int64_t max_pairs,
                                        int64_t* out_id_a, int64_t* out_id_b, float* out_scores, int64_t* out_count,
                                        int64_t* out_total) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "find_duplicates: searcher is NULL");
        PCV_REQUIRE(out_id_a != nullptr && out_id_b != nullptr && out_count != nullptr, "find_duplicates: out_id_a, out_id_b or out_count is NULL");
        PCV_REQUIRE(max_pairs >= 1 && max_pairs <= (int64_t)PCV_MAX_DUPLICATE_PAIRS, "find_duplicates: max_pairs %lld outside [1,%d]",
                    (long long)max_pairs, (int)PCV_MAX_DUPLICATE_PAIRS);
        PCV_REQUIRE(threshold == threshold, "find_duplicates: threshold is NaN");
        PCV_REQUIRE(threshold > -1.0f && threshold <= 1.0f, "find_duplicates: threshold %g outside (-1, 1]", (double)threshold);
        const auto lk = enter(s, "find_duplicates");
        find_duplicates(s, source_ids, n_sources, threshold, max_pairs, out_id_a, out_id_b, out_scores, out_count, out_total);
    });
}

// (a view reads its parent's table: the parent stays locked while the kernels may follow its pointers — pcv_searcher_search_grouped)
static std::unique_lock<std::mutex> lock_group_owner(pcv_searcher* s) {
    return s->view_parent ? std::unique_lock<std::mutex>(s->view_parent->mu) : std::unique_lock<std::mutex>();
}

pcv_status pcv_searcher_find_duplicates_grouped(pcv_searcher* s, const int64_t* source_ids, int n_sources, float threshold, int64_t max_pairs,
                                                int64_t* out_id_a, int64_t* out_id_b, float* out_scores, int64_t* out_count,
                                                int64_t* out_total, int64_t* out_skipped) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "find_duplicates_grouped: searcher is NULL");
        PCV_REQUIRE(out_id_a != nullptr && out_id_b != nullptr && out_count != nullptr,
                    "find_duplicates_grouped: out_id_a, out_id_b or out_count is NULL");
        PCV_REQUIRE(max_pairs >= 1 && max_pairs <= (int64_t)PCV_MAX_DUPLICATE_PAIRS, "find_duplicates_grouped: max_pairs %lld outside [1,%d]",
                    (long long)max_pairs, (int)PCV_MAX_DUPLICATE_PAIRS);
        PCV_REQUIRE(threshold == threshold, "find_duplicates_grouped: threshold is NaN");
        PCV_REQUIRE(threshold > -1.0f && threshold <= 1.0f, "find_duplicates_grouped: threshold %g outside (-1, 1]", (double)threshold);
        const auto lk = enter(s, "find_duplicates_grouped");
        const auto plk = lock_group_owner(s);
        find_duplicates(s, source_ids, n_sources, threshold, max_pairs, out_id_a, out_id_b, out_scores, out_count, out_total,
                        s->view_parent ? s->view_parent : s, out_skipped);
    });
}

pcv_status pcv_searcher_last_pair_group_stats(pcv_searcher* s, pcv_pair_group_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_pair_group_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->pair_group_stats;
    });
}

pcv_status pcv_searcher_last_duplicate_stats(pcv_searcher* s, pcv_duplicate_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_duplicate_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->dup_stats;
    });
}

pcv_status pcv_searcher_assign(pcv_searcher* s, const float* labels, int n_labels, const int64_t* source_ids, int n_sources, int64_t capacity,
                               int32_t* out_label, float* out_score, int64_t* out_ids, int64_t* out_counts, int64_t* out_n) {
    return guarded([&] {
        PCV_REQUIRE(labels != nullptr && out_n != nullptr, "assign: labels or out_n is NULL");
        PCV_REQUIRE(n_labels >= 1 && n_labels <= (int)PCV_MAX_LABELS, "assign: %d labels, outside [1,%d]", n_labels, (int)PCV_MAX_LABELS);
        PCV_REQUIRE(capacity >= 0 && (out_label != nullptr || capacity == 0), "assign: out_label is NULL with capacity %lld", (long long)capacity);
        PCV_REQUIRE(s != nullptr, "assign: searcher is NULL");
        const auto lk = enter(s, "assign");
        assign_or_kmeans(s, "assign", labels, n_labels, 0, s->metric, source_ids, n_sources, capacity, nullptr, out_label, out_score, out_ids, out_counts,
                         nullptr, nullptr, out_n);
    });
}

pcv_status pcv_searcher_kmeans(pcv_searcher* s, const float* init, int n_labels, int max_iters, const int64_t* source_ids, int n_sources,
                               int64_t capacity, float* out_centroids, int32_t* out_label, float* out_score, int64_t* out_ids,
                               int64_t* out_counts, int32_t* out_iters, int64_t* out_moved, int64_t* out_n) {
    return guarded([&] {
        PCV_REQUIRE(init != nullptr && out_n != nullptr, "kmeans: init or out_n is NULL");
        PCV_REQUIRE(n_labels >= 1 && n_labels <= (int)PCV_MAX_LABELS, "kmeans: %d centroids, outside [1,%d]", n_labels, (int)PCV_MAX_LABELS);
        PCV_REQUIRE(max_iters >= 0, "kmeans: max_iters %d is negative", max_iters);
        PCV_REQUIRE(capacity >= 0 && (out_label != nullptr || capacity == 0), "kmeans: out_label is NULL with capacity %lld", (long long)capacity);
        PCV_REQUIRE(out_centroids != nullptr || (out_label == nullptr && capacity == 0), "kmeans: out_centroids is NULL");
        PCV_REQUIRE(s != nullptr, "kmeans: searcher is NULL");
        const auto lk = enter(s, "kmeans");
        assign_or_kmeans(s, "kmeans", init, n_labels, max_iters, PCV_METRIC_COSINE, source_ids, n_sources, capacity, out_centroids, out_label, out_score,
                         out_ids, out_counts, out_iters, out_moved, out_n);
    });
}

pcv_status pcv_searcher_label_sums(pcv_searcher* s, const int64_t* source_ids, int n_sources, const int32_t* labels, int64_t n, int n_labels,
                                   int64_t* out_sums, int64_t* out_counts) {
    return guarded([&] {
        PCV_REQUIRE(out_sums != nullptr && n >= 0 && (labels != nullptr || n == 0), "label_sums: labels or out_sums is NULL");
        PCV_REQUIRE(n_labels >= 1 && n_labels <= (int)PCV_MAX_LABELS, "label_sums: %d labels, outside [1,%d]", n_labels, (int)PCV_MAX_LABELS);
        PCV_REQUIRE(s != nullptr, "label_sums: searcher is NULL");
        const auto lk = enter(s, "label_sums");
        label_sums(s, source_ids, n_sources, labels, n, n_labels, out_sums, out_counts);
    });
}

pcv_status pcv_searcher_last_assign_stats(pcv_searcher* s, pcv_assign_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_assign_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->assign_stats;
    });
}

pcv_status pcv_searcher_assign_top(pcv_searcher* s, const float* labels, int n_labels, int m, float min_score, const int64_t* source_ids,
                                   int n_sources, int64_t capacity, int32_t* out_labels, float* out_scores, int64_t* out_ids, int32_t* out_counts,
                                   int64_t* out_label_rows, int64_t* out_n) {
    return guarded([&] {
        PCV_REQUIRE(labels != nullptr && out_n != nullptr, "assign_top: labels or out_n is NULL");
        PCV_REQUIRE(n_labels >= 1 && n_labels <= (int)PCV_MAX_LABELS, "assign_top: %d labels, outside [1,%d]", n_labels, (int)PCV_MAX_LABELS);
        PCV_REQUIRE(m >= 1 && m <= (int)PCV_MAX_TOP_LABELS, "assign_top: m %d outside [1,%d]", m, (int)PCV_MAX_TOP_LABELS);
        PCV_REQUIRE(min_score == min_score, "assign_top: min_score is NaN");
        PCV_REQUIRE(capacity >= 0 && (out_labels != nullptr || capacity == 0), "assign_top: out_labels is NULL with capacity %lld", (long long)capacity);
        PCV_REQUIRE(out_counts != nullptr || (out_labels == nullptr && capacity == 0), "assign_top: out_counts is NULL");
        PCV_REQUIRE(s != nullptr, "assign_top: searcher is NULL");
        const auto lk = enter(s, "assign_top");
        assign_top(s, labels, n_labels, m, min_score, source_ids, n_sources, capacity, out_labels, out_scores, out_ids, out_counts, out_label_rows,
                   out_n);
    });
}

pcv_status pcv_searcher_last_assign_top_stats(pcv_searcher* s, pcv_assign_top_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_assign_top_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->assign_top_stats;
    });
}

pcv_status pcv_searcher_neighbors(pcv_searcher* s, const int64_t* source_ids, int n_sources, int k, int64_t capacity, int64_t* out_ids,
                                  int64_t* out_neighbor_ids, float* out_scores, int32_t* out_counts, int64_t* out_rows) {
    return guarded([&] {
        PCV_REQUIRE(out_rows != nullptr, "neighbors: out_rows is NULL");
        PCV_REQUIRE(k >= 1 && k <= (int)PCV_MAX_NEIGHBORS, "neighbors: k %d outside [1,%d]", k, (int)PCV_MAX_NEIGHBORS);
        PCV_REQUIRE(capacity >= 0, "neighbors: capacity %lld is negative", (long long)capacity);
        const bool all = out_ids != nullptr && out_neighbor_ids != nullptr && out_scores != nullptr && out_counts != nullptr;
        const bool none = out_ids == nullptr && out_neighbor_ids == nullptr && out_scores == nullptr && out_counts == nullptr;
        PCV_REQUIRE(all || (none && capacity == 0), "neighbors: an output array is NULL with capacity %lld", (long long)capacity);
        PCV_REQUIRE(s != nullptr, "neighbors: searcher is NULL");
        const auto lk = enter(s, "neighbors");
        neighbors(s, source_ids, n_sources, k, capacity, out_ids, out_neighbor_ids, out_scores, out_counts, out_rows);
    });
}

pcv_status pcv_searcher_neighbors_grouped(pcv_searcher* s, const int64_t* source_ids, int n_sources, int k, uint32_t flags, int64_t capacity,
                                          int64_t* out_ids, int64_t* out_neighbor_ids, float* out_scores, int64_t* out_neighbor_groups,
                                          int32_t* out_counts, int64_t* out_rows) {
    return guarded([&] {
        PCV_REQUIRE(flags <= (uint32_t)(PCV_GROUPS_SKIP_OWN | PCV_GROUPS_ONE_PER_GROUP), "neighbors_grouped: flags %#x outside 0..3", flags);
        PCV_REQUIRE(out_rows != nullptr, "neighbors_grouped: out_rows is NULL");
        PCV_REQUIRE(k >= 1 && k <= (int)PCV_MAX_NEIGHBORS, "neighbors_grouped: k %d outside [1,%d]", k, (int)PCV_MAX_NEIGHBORS);
        PCV_REQUIRE(capacity >= 0, "neighbors_grouped: capacity %lld is negative", (long long)capacity);
        const bool all = out_ids != nullptr && out_neighbor_ids != nullptr && out_scores != nullptr && out_counts != nullptr;
        const bool none = out_ids == nullptr && out_neighbor_ids == nullptr && out_scores == nullptr && out_counts == nullptr &&
                          out_neighbor_groups == nullptr;
        PCV_REQUIRE(all || (none && capacity == 0), "neighbors_grouped: an output array is NULL with capacity %lld", (long long)capacity);
        PCV_REQUIRE(s != nullptr, "neighbors_grouped: searcher is NULL");
        const auto lk = enter(s, "neighbors_grouped");
        const auto plk = lock_group_owner(s);
        neighbors(s, source_ids, n_sources, k, capacity, out_ids, out_neighbor_ids, out_scores, out_counts, out_rows,
                  s->view_parent ? s->view_parent : s, flags, out_neighbor_groups);
    });
}

pcv_status pcv_searcher_last_neighbor_stats(pcv_searcher* s, pcv_neighbor_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_neighbor_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->nbr_stats;
    });
}

pcv_status pcv_searcher_match(pcv_searcher* s, const int64_t* from_source_ids, int n_from, const int64_t* to_source_ids, int n_to, int k,
                              float min_score, int64_t capacity, int64_t* out_ids, int64_t* out_match_ids, float* out_scores,
                              int32_t* out_counts, int64_t* out_rows) {
    return guarded([&] {
        PCV_REQUIRE(out_rows != nullptr, "match: out_rows is NULL");
        PCV_REQUIRE(k >= 1 && k <= (int)PCV_MAX_NEIGHBORS, "match: k %d outside [1,%d]", k, (int)PCV_MAX_NEIGHBORS);
        PCV_REQUIRE(min_score == min_score, "match: min_score is NaN");
        PCV_REQUIRE(min_score >= -1.0f && min_score <= 1.0f, "match: min_score %g outside [-1, 1]", (double)min_score);
        PCV_REQUIRE(capacity >= 0, "match: capacity %lld is negative", (long long)capacity);
        const bool all = out_ids != nullptr && out_match_ids != nullptr && out_scores != nullptr && out_counts != nullptr;
        const bool none = out_ids == nullptr && out_match_ids == nullptr && out_scores == nullptr && out_counts == nullptr;
        PCV_REQUIRE(all || (none && capacity == 0), "match: an output array is NULL with capacity %lld", (long long)capacity);
        PCV_REQUIRE(s != nullptr, "match: searcher is NULL");
        const auto lk = enter(s, "match");
        match(s, from_source_ids, n_from, to_source_ids, n_to, k, min_score, capacity, out_ids, out_match_ids, out_scores, out_counts, out_rows);
    });
}

pcv_status pcv_searcher_match_grouped(pcv_searcher* s, const int64_t* from_source_ids, int n_from, const int64_t* to_source_ids, int n_to, int k,
                                      float min_score, uint32_t flags, int64_t capacity, int64_t* out_ids, int64_t* out_match_ids,
                                      float* out_scores, int64_t* out_match_groups, int32_t* out_counts, int64_t* out_rows) {
    return guarded([&] {
        PCV_REQUIRE(flags <= (uint32_t)(PCV_GROUPS_SKIP_OWN | PCV_GROUPS_ONE_PER_GROUP), "match_grouped: flags %#x outside 0..3", flags);
        PCV_REQUIRE(out_rows != nullptr, "match_grouped: out_rows is NULL");
        PCV_REQUIRE(k >= 1 && k <= (int)PCV_MAX_NEIGHBORS, "match_grouped: k %d outside [1,%d]", k, (int)PCV_MAX_NEIGHBORS);
        PCV_REQUIRE(min_score == min_score, "match_grouped: min_score is NaN");
        PCV_REQUIRE(min_score >= -1.0f && min_score <= 1.0f, "match_grouped: min_score %g outside [-1, 1]", (double)min_score);
        PCV_REQUIRE(capacity >= 0, "match_grouped: capacity %lld is negative", (long long)capacity);
        const bool all = out_ids != nullptr && out_match_ids != nullptr && out_scores != nullptr && out_counts != nullptr;
        const bool none = out_ids == nullptr && out_match_ids == nullptr && out_scores == nullptr && out_counts == nullptr &&
                          out_match_groups == nullptr;
        PCV_REQUIRE(all || (none && capacity == 0), "match_grouped: an output array is NULL with capacity %lld", (long long)capacity);
        PCV_REQUIRE(s != nullptr, "match_grouped: searcher is NULL");
        const auto lk = enter(s, "match_grouped");
        const auto plk = lock_group_owner(s);
        match(s, from_source_ids, n_from, to_source_ids, n_to, k, min_score, capacity, out_ids, out_match_ids, out_scores, out_counts, out_rows,
              s->view_parent ? s->view_parent : s, flags, out_match_groups);
    });
}

pcv_status pcv_searcher_last_match_stats(pcv_searcher* s, pcv_match_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_match_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->match_stats;
    });
}

pcv_status pcv_searcher_density_clusters(pcv_searcher* s, const int64_t* source_ids, int n_sources, float threshold, int min_items,
                                         int64_t capacity, int64_t* out_ids, int32_t* out_label, int8_t* out_kind, int32_t* out_degree,
                                         int64_t* out_rows, int32_t* out_clusters) {
    return guarded([&] {
        PCV_REQUIRE(out_rows != nullptr, "density_clusters: out_rows is NULL");
        PCV_REQUIRE(threshold == threshold, "density_clusters: threshold is NaN");
        PCV_REQUIRE(threshold > -1.0f && threshold <= 1.0f, "density_clusters: threshold %g outside (-1, 1]", (double)threshold);
        PCV_REQUIRE(min_items >= 1, "density_clusters: min_items %d is below 1", min_items);
        PCV_REQUIRE(capacity >= 0, "density_clusters: capacity %lld is negative", (long long)capacity);
        const bool all = out_label != nullptr && out_kind != nullptr && out_clusters != nullptr;
        const bool none = out_label == nullptr && out_kind == nullptr && out_degree == nullptr && out_ids == nullptr;
        PCV_REQUIRE(all || (none && capacity == 0), "density_clusters: out_label, out_kind or out_clusters is NULL with capacity %lld",
                    (long long)capacity);
        PCV_REQUIRE(s != nullptr, "density_clusters: searcher is NULL");
        const auto lk = enter(s, "density_clusters");
        density_clusters(s, source_ids, n_sources, threshold, min_items, capacity, out_ids, out_label, out_kind, out_degree, out_rows, out_clusters);
    });
}

pcv_status pcv_searcher_last_density_stats(pcv_searcher* s, pcv_density_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_density_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->density_stats;
    });
}

pcv_status pcv_searcher_linkage_tree(pcv_searcher* s, const int64_t* source_ids, int n_sources, int64_t capacity, int64_t* out_ids,
                                     int8_t* out_part, int64_t* out_pos_a, int64_t* out_pos_b, int64_t* out_id_a, int64_t* out_id_b,
                                     double* out_c, int64_t* out_rows, int64_t* out_edges) {
    return guarded([&] {
        PCV_REQUIRE(out_rows != nullptr, "linkage_tree: out_rows is NULL");
        PCV_REQUIRE(capacity >= 0, "linkage_tree: capacity %lld is negative", (long long)capacity);
        const bool all = out_pos_a != nullptr && out_pos_b != nullptr && out_c != nullptr && out_edges != nullptr;
        const bool none = out_pos_a == nullptr && out_pos_b == nullptr && out_c == nullptr && out_ids == nullptr && out_part == nullptr &&
                          out_id_a == nullptr && out_id_b == nullptr;
        PCV_REQUIRE(all || (none && capacity == 0), "linkage_tree: out_pos_a, out_pos_b, out_c or out_edges is NULL with capacity %lld",
                    (long long)capacity);
        PCV_REQUIRE((out_id_a == nullptr) == (out_id_b == nullptr), "linkage_tree: one of out_id_a and out_id_b is NULL, the other is not");
        PCV_REQUIRE(s != nullptr, "linkage_tree: searcher is NULL");
        const auto lk = enter(s, "linkage_tree");
        linkage_tree(s, source_ids, n_sources, capacity, out_ids, out_part, out_pos_a, out_pos_b, out_id_a, out_id_b, out_c, out_rows, out_edges);
    });
}

pcv_status pcv_searcher_last_linkage_stats(pcv_searcher* s, pcv_linkage_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_linkage_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->linkage_stats;
    });
}

pcv_status pcv_searcher_reach_tree(pcv_searcher* s, const int64_t* source_ids, int n_sources, int min_items, int64_t capacity, int64_t* out_ids,
                                   int8_t* out_part, double* out_core, int64_t* out_pos_a, int64_t* out_pos_b, int64_t* out_id_a, int64_t* out_id_b,
                                   double* out_w, double* out_c, int64_t* out_rows, int64_t* out_edges) {
    return guarded([&] {
        PCV_REQUIRE(out_rows != nullptr, "reach_tree: out_rows is NULL");
        PCV_REQUIRE(min_items >= 1 && min_items <= (int)PCV_MAX_NEIGHBORS + 1, "reach_tree: min_items %d outside [1,%d]", min_items,
                    (int)PCV_MAX_NEIGHBORS + 1);
        PCV_REQUIRE(capacity >= 0, "reach_tree: capacity %lld is negative", (long long)capacity);
        const bool all = out_pos_a != nullptr && out_pos_b != nullptr && out_w != nullptr && out_edges != nullptr;
        const bool none = out_pos_a == nullptr && out_pos_b == nullptr && out_w == nullptr && out_c == nullptr && out_ids == nullptr &&
                          out_part == nullptr && out_core == nullptr && out_id_a == nullptr && out_id_b == nullptr;
        PCV_REQUIRE(all || (none && capacity == 0), "reach_tree: out_pos_a, out_pos_b, out_w or out_edges is NULL with capacity %lld",
                    (long long)capacity);
        PCV_REQUIRE((out_id_a == nullptr) == (out_id_b == nullptr), "reach_tree: one of out_id_a and out_id_b is NULL, the other is not");
        PCV_REQUIRE(s != nullptr, "reach_tree: searcher is NULL");
        const auto lk = enter(s, "reach_tree");
        reach_tree(s, source_ids, n_sources, min_items, capacity, out_ids, out_part, out_core, out_pos_a, out_pos_b, out_id_a, out_id_b, out_w, out_c,
                   out_rows, out_edges);
    });
}

pcv_status pcv_searcher_last_reach_stats(pcv_searcher* s, pcv_reach_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_reach_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->reach_stats;
    });
}

// Union-find over the positions: the smaller root wins, so a component's root is its lowest position, and numbering the roots in
// ascending order numbers the clusters by their lowest position.
pcv_status pcv_linkage_cut(const int64_t* pos_a, const int64_t* pos_b, const double* c, int64_t n_edges, const int8_t* part, int64_t n_rows,
                           double threshold, int64_t min_clusters, int32_t* out_label, int32_t* out_clusters) {
    return guarded([&] {
        PCV_REQUIRE(n_edges >= 0 && n_rows >= 0, "linkage_cut: %lld edges, %lld rows", (long long)n_edges, (long long)n_rows);
        PCV_REQUIRE(n_edges == 0 || (pos_a != nullptr && pos_b != nullptr && c != nullptr), "linkage_cut: %lld edges without their arrays", (long long)n_edges);
        PCV_REQUIRE(n_rows == 0 || out_label != nullptr, "linkage_cut: out_label is NULL");
        PCV_REQUIRE(n_rows <= (int64_t)INT32_MAX, "linkage_cut: %lld rows do not fit the int32 labels", (long long)n_rows);
        PCV_REQUIRE(threshold == threshold, "linkage_cut: threshold is NaN");
        PCV_REQUIRE(min_clusters >= 1, "linkage_cut: min_clusters %lld is below 1", (long long)min_clusters);
        for (int64_t i = 0; i < n_edges; ++i) {
            PCV_REQUIRE(pos_a[i] >= 0 && pos_a[i] < pos_b[i] && pos_b[i] < n_rows, "linkage_cut: edge %lld joins positions %lld and %lld of %lld rows",
                        (long long)i, (long long)pos_a[i], (long long)pos_b[i], (long long)n_rows);
            PCV_REQUIRE(c[i] == c[i] && (i == 0 || c[i] <= c[i - 1]), "linkage_cut: the edges are not ordered from best to worst at edge %lld", (long long)i);
            PCV_REQUIRE(part == nullptr || (part[pos_a[i]] != 0 && part[pos_b[i]] != 0), "linkage_cut: edge %lld has an end that takes no part", (long long)i);
        }
        std::vector<int64_t> parent((size_t)n_rows);
        std::iota(parent.begin(), parent.end(), (int64_t)0);
        auto find = [&](int64_t i) {
            while (parent[(size_t)i] != i) i = parent[(size_t)i] = parent[(size_t)parent[(size_t)i]];
            return i;
        };
        const int64_t keep_below = n_edges - (min_clusters - 1);
        for (int64_t i = 0; i < n_edges && i < keep_below; ++i) {
            if (!(c[i] >= threshold)) break;  // (c does not rise again)
            const int64_t x = find(pos_a[i]), y = find(pos_b[i]);
            if (x != y) parent[(size_t)std::max(x, y)] = std::min(x, y);
        }
        int32_t clusters = 0;
        for (int64_t r = 0; r < n_rows; ++r) {  // a root comes before every other row of its component
            if (part != nullptr && part[r] == 0)
                out_label[r] = -1;
            else if (parent[(size_t)r] == r)
                out_label[r] = clusters++;
            else
                out_label[r] = out_label[find(r)];
        }
        if (out_clusters) *out_clusters = clusters;
    });
}

pcv_status pcv_searcher_seeds(pcv_searcher* s, const int64_t* source_ids, int n_sources, int k, int method, uint64_t seed,
                              const int64_t* first_id, int64_t* out_ids, int64_t* out_positions, int64_t* out_totals,
                              float* out_cover, int32_t* out_count) {
    return guarded([&] {
        PCV_REQUIRE(out_ids != nullptr && out_positions != nullptr && out_totals != nullptr && out_cover != nullptr && out_count != nullptr,
                    "seeds: an output is NULL");
        PCV_REQUIRE(k >= 1 && k <= (int)PCV_MAX_SEEDS, "seeds: k %d outside [1,%d]", k, (int)PCV_MAX_SEEDS);
        PCV_REQUIRE(method == PCV_SEED_FARTHEST || method == PCV_SEED_KMEANSPP, "seeds: method %d is neither PCV_SEED_FARTHEST nor PCV_SEED_KMEANSPP", method);
        PCV_REQUIRE(s != nullptr, "seeds: searcher is NULL");
        const auto lk = enter(s, "seeds");
        seeds(s, source_ids, n_sources, k, method, seed, first_id, out_ids, out_positions, out_totals, out_cover, out_count);
    });
}

pcv_status pcv_searcher_last_seed_stats(pcv_searcher* s, pcv_seed_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_seed_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->seed_stats;
    });
}

pcv_status pcv_seed_draw(uint64_t seed, int step, uint64_t total, uint64_t* out_t) {
    return guarded([&] {
        PCV_REQUIRE(out_t != nullptr, "seed_draw: out_t is NULL");
        PCV_REQUIRE(step >= 0, "seed_draw: step %d is negative", step);
        PCV_REQUIRE(total != 0, "seed_draw: total is 0");
        *out_t = seed_draw(seed, (uint32_t)step, total);
    });
}

pcv_status pcv_searcher_moments(pcv_searcher* s, const int64_t* source_ids, int n_sources, int centered, int64_t* out_sums, double* out_matrix,
                                int64_t* out_n) {
    return guarded([&] {
        PCV_REQUIRE(out_sums != nullptr && out_n != nullptr, "moments: out_sums or out_n is NULL");
        PCV_REQUIRE(s != nullptr, "moments: searcher is NULL");
        const auto lk = enter(s, "moments");
        moments(s, source_ids, n_sources, centered, out_sums, out_matrix, out_n);
    });
}

pcv_status pcv_searcher_last_moment_stats(pcv_searcher* s, pcv_moment_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_moment_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->moment_stats;
    });
}

pcv_status pcv_searcher_principal_axes(pcv_searcher* s, const int64_t* source_ids, int n_sources, int m, float* out_axes, double* out_offsets,
                                       double* out_variance, int64_t* out_n) {
    return guarded([&] {
        PCV_REQUIRE(out_axes != nullptr && out_offsets != nullptr && out_variance != nullptr && out_n != nullptr, "principal_axes: an output is NULL");
        PCV_REQUIRE(m >= 1 && m <= (int)PCV_MAX_AXES, "principal_axes: m %d outside [1,%d]", m, (int)PCV_MAX_AXES);
        PCV_REQUIRE(s != nullptr, "principal_axes: searcher is NULL");
        const auto lk = enter(s, "principal_axes");
        principal_axes(s, source_ids, n_sources, m, out_axes, out_offsets, out_variance, out_n);
    });
}

pcv_status pcv_searcher_project(pcv_searcher* s, const float* axes, const double* offsets, int m, const int64_t* source_ids, int n_sources,
                                int64_t capacity, float* out_coords, int64_t* out_ids, int64_t* out_n) {
    return guarded([&] {
        PCV_REQUIRE(axes != nullptr && out_n != nullptr, "project: axes or out_n is NULL");
        PCV_REQUIRE(m >= 1 && m <= (int)PCV_MAX_AXES, "project: m %d outside [1,%d]", m, (int)PCV_MAX_AXES);
        PCV_REQUIRE(capacity >= 0 && (out_coords != nullptr || capacity == 0), "project: out_coords is NULL with capacity %lld", (long long)capacity);
        PCV_REQUIRE(out_coords != nullptr || out_ids == nullptr, "project: out_ids without out_coords");
        PCV_REQUIRE(s != nullptr, "project: searcher is NULL");
        // (the dimension is fixed when the searcher is created: reading it needs no lock)
        for (int64_t i = 0; i < (int64_t)m * s->D; ++i) PCV_REQUIRE(std::isfinite(axes[i]), "project: axis %lld has a value that is not finite", (long long)(i / s->D));
        for (int j = 0; offsets && j < m; ++j) PCV_REQUIRE(std::isfinite(offsets[j]), "project: offset %d is not finite", j);
        const auto lk = enter(s, "project");
        project(s, axes, offsets, m, source_ids, n_sources, capacity, out_coords, out_ids, out_n);
    });
}

pcv_status pcv_searcher_last_project_stats(pcv_searcher* s, pcv_project_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "last_project_stats: NULL argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *out = s->project_stats;
    });
}

// Union-find over the distinct ids of the pairs, by their index in ascending order: a root is always the smallest index of its
// component, so the label of a component is its smallest id.
pcv_status pcv_duplicate_groups(const int64_t* id_a, const int64_t* id_b, int64_t n_pairs, int64_t* out_ids, int64_t* out_group,
                                int64_t capacity, int64_t* out_n_ids) {
    return guarded([&] {
        PCV_REQUIRE(out_n_ids != nullptr, "duplicate_groups: out_n_ids is NULL");
        PCV_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || (id_a != nullptr && id_b != nullptr)), "duplicate_groups: %lld pairs without their ids",
                    (long long)n_pairs);
        std::vector<int64_t> ids;
        ids.reserve((size_t)n_pairs * 2);
        ids.insert(ids.end(), id_a, id_a + n_pairs);
        ids.insert(ids.end(), id_b, id_b + n_pairs);
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        const int64_t n = (int64_t)ids.size();
        *out_n_ids = n;
        PCV_REQUIRE(capacity >= n, "duplicate_groups: %lld ids, room for %lld", (long long)n, (long long)capacity);
        PCV_REQUIRE(n == 0 || (out_ids != nullptr && out_group != nullptr), "duplicate_groups: out_ids or out_group is NULL");
        std::vector<int64_t> parent((size_t)n);
        std::iota(parent.begin(), parent.end(), (int64_t)0);
        auto find = [&](int64_t i) {
            while (parent[(size_t)i] != i) i = parent[(size_t)i] = parent[(size_t)parent[(size_t)i]];
            return i;
        };
        for (int64_t k = 0; k < n_pairs; ++k) {
            const int64_t x = find(std::lower_bound(ids.begin(), ids.end(), id_a[k]) - ids.begin());
            const int64_t y = find(std::lower_bound(ids.begin(), ids.end(), id_b[k]) - ids.begin());
            if (x != y) parent[(size_t)std::max(x, y)] = std::min(x, y);
        }
        for (int64_t i = 0; i < n; ++i) {
            out_ids[i] = ids[(size_t)i];
            out_group[i] = ids[(size_t)find(i)];
        }
    });
}

}  // extern "C"
