// searcher_pass.cpp — the scan pass pipeline: enqueue_pass and finish_pass with their steps, the captured graph of a pass, and
// what a search call settles before its first pass.  One unit, so that the steps of a pass inline into each other.  Called by
// the search calls (searcher_calls.cpp, searcher_exchange.cpp, searcher.cpp) with s->mu held; interface: searcher_pass.h.
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "searcher_pass.h"

namespace pcv {

void ensure_workspace(pcv_searcher* s) {
    const size_t Q = kMfmaQueries;
    s->d_qf32.ensure(Q * s->Dp);
    s->d_qraw.ensure(Q * s->Dp);
    s->d_qbf16.ensure(Q * s->Dp);
    s->d_q8.ensure(Q * (size_t)((s->Dp + 127) & ~127));
    s->d_q8c.ensure(Q * 8);  // (the int8 test's constants, then the 6-bit test's: scan.h)
    s->d_spec.ensure(Q);
    s->d_margin.ensure(Q);
    s->d_margin32.ensure(Q);
    s->d_tau.ensure((Q + 1) * kHot);  // (+ the side-by-side copy of the thresholds: ScanParams::tau_c)
    s->d_slots.ensure(Q * kMaxK);
    s->d_cnt.ensure(Q * kHot);
    s->d_cand.ensure(Q * s->cand_cap);
    s->d_cand_s.ensure(Q * s->cand_cap);
    s->d_hits.ensure(Q * kMaxK);
    s->pin.ensure(1);
    for (auto& e : s->ev)
        if (!e) PCV_HIP(hipEventCreate(&e));
}

namespace {

constexpr int64_t kGraphRows = (int64_t)4 << 20;  // passes over more rows than this are not replayed as graphs

// offsets inside the pass block
struct PassLayout {
    size_t off_seg, off_ceil, off_range, off_q, total;
};
// `with_ceil`: the pass has ceilings (scan.h, CeilRec: a search for more than kMaxK results) — their records sit between the
// segment table and the queries, so that they travel with every attempt of the pass
PassLayout pass_layout(const pcv_searcher* s, size_t nseg, bool with_ceil) {
    PassLayout L;
    L.off_seg = align_up(sizeof(ScanParams));
    L.off_ceil = align_up(L.off_seg + nseg * sizeof(SegDesc));
    // (... and behind them the bounds and thresholds of a range pass, which is a pass under ceilings: scan.h, RangeRec)
    L.off_range = with_ceil ? align_up(L.off_ceil + (size_t)kMfmaQueries * sizeof(CeilRec)) : L.off_ceil;
    L.off_q = with_ceil ? align_up(L.off_range + (size_t)kMfmaQueries * sizeof(RangeRec)) : L.off_ceil;
    L.total = L.off_q + (size_t)kMfmaQueries * s->D * sizeof(float);
    return L;
}
void ensure_pass_block(pcv_searcher* s, size_t nseg) {
    const size_t want = pass_layout(s, nseg, true).total;
    if (want <= s->pin_pass.n && want <= s->d_pass.n) return;
    PCV_HIP(hipStreamSynchronize(s->ctx->stream));
    const size_t cap = want + want / 2;
    s->pin_pass.ensure(cap);
    s->d_pass.ensure(cap);
}

// ---- enqueue_pass, step by step ----
// 1. What the pass streams, decided while the segment table is filled.
struct PassSource {
    int src_kind = 0;      // 0 f32 rows, 1 bf16 copies, 2 int8 copies
    bool have_mid = false; // every selected segment has its mid copy, and the pass uses it
    bool six = false;      // the 6-bit copies are streamed in place of the int8 ones
    uint32_t flags = 0;    // ScanParams::flags of the pass: the tuning word with the searcher's own bits (scan.h) set to this decision
    uint32_t total_blocks = 0;
    int64_t rows = 0;
};
// The rule is here and nowhere else: a copy is streamed iff the searcher keeps that kind, EVERY selected segment has it and it
// covers EVERY row of each (a copy that does not cover every row yet is not used).
PassSource fill_segment_table(const pcv_searcher* s, const PassRequest& r, SegDesc* tab) {
    PassSource src;
    src.src_kind = (r.kernel == PCV_KERNEL_MFMA) ? copy_kind_wanted(s) : 0;
    if (src.src_kind == 2 && (mfma8_pass_queries(s->Dp) < r.B || s->Dp > 1024)) src.src_kind = 0;
    const int src_wanted = src.src_kind;
    bool have_mid = true, have_six = true;
    uint32_t blk0 = 0;
    for (int i = 0; i < r.nseg; ++i) {
        const Segment& g = *r.segs[i].g;
        const bool mid = g.mid16 != nullptr && g.mid_rows >= g.nrows;
        tab[i] = SegDesc{g.blk, g.scale, g.ids, g.id0, g.pos0, g.nrows, g.nblocks(), blk0, 0, g.blk16, g.blk8, mid ? g.mid16 : nullptr, mid ? g.scale16 : nullptr, g.scale8,
                         g.blk6, g.scale6};
        have_six = have_six && g.blk6 != nullptr && g.six_rows >= g.nrows;
        have_mid = have_mid && mid;
        if ((src.src_kind == 1 ? g.blk16 == nullptr : (src.src_kind == 2 ? g.blk8 == nullptr : false)) || g.copied_rows < g.nrows) src.src_kind = 0;
        PCV_REQUIRE((uint64_t)blk0 + g.nblocks() < 0xffffff00ull, "search: more than 2^32 row blocks in one launch");
        blk0 += g.nblocks();
        src.rows += g.nrows;
    }
    if (src.src_kind != 2) {
        // the mid screen's bound uses |q'|_1, which only the int8 path's quantize_queries_kernel computes: passes that stream
        // the bf16 copy or the f32 rows (few coarse survivors anyway) go straight to the f32 row
        for (int i = 0; i < r.nseg; ++i) {
            tab[i].mid16 = nullptr;
            tab[i].scale16 = nullptr;
        }
        have_mid = false;
    }
    PCV_REQUIRE(r.B <= 128 || (r.kernel == PCV_KERNEL_MFMA && src.src_kind == 2 && src_wanted == 2), "search: %d queries in one pass without int8 copies of every selected row", r.B);
    src.total_blocks = blk0;
    src.have_mid = have_mid && r.nseg > 0;
    src.flags = (s->scan_flags & ~kFlagsSearcherOwned) | (src.src_kind == 1 ? kFlagSrc16 : 0u) | (src.src_kind == 2 ? kFlagSrc8 : 0u);
    // the 6-bit copies: AUTO's kernel choice only (PCV_KERNEL_MFMA pins the whole-int8 scan), 5..64 queries (scan.h)
    src.six = src.src_kind == 2 && have_six && r.nseg > 0 && s->kernel == PCV_KERNEL_AUTO && !(s->scan_flags & kTuneNoSix) &&
              mfma8_six_pass(r.B, s->Dp, src.flags, r.nseg);
    if (src.six) src.flags |= kFlagSix;
    return src;
}

// 2. The parameters of a top-k pass, from the workspace (a range pass: fill_range_part on top).  No guess yet.
void fill_params(pcv_searcher* s, const PassRequest& r, const PassLayout& L, const PassSource& src, ScanParams& p) {
    p = ScanParams{};
    p.seg = reinterpret_cast<const SegDesc*>(s->d_pass.p + L.off_seg);
    p.nseg = r.nseg;
    p.total_blocks = src.total_blocks;
    p.D = s->D;
    p.D4 = s->D4;
    p.B = r.B;
    p.k = r.k();
    p.metric = s->metric;
    p.tile_rows = r.kernel == PCV_KERNEL_MFMA ? mfma_tile_rows(r.B) : 0u;
    p.queries = reinterpret_cast<const float*>(s->d_pass.p + L.off_q);
    if (r.kind == PassRequest::kCeilings) {
        std::memcpy(s->pin_pass.p + L.off_ceil, r.topk.ceil, (size_t)r.B * sizeof(CeilRec));
        p.ceil = reinterpret_cast<const CeilRec*>(s->d_pass.p + L.off_ceil);
    }
    p.qf32 = s->d_qf32.p;
    p.qbf16 = s->d_qbf16.p;
    p.q8 = s->d_q8.p;
    p.q8c = s->d_q8c.p;
    p.qraw = s->d_qraw.p;
    p.margin = s->d_margin.p;
    p.margin32 = s->d_margin32.p;
    p.tau = s->d_tau.p;
    p.tau_c = s->d_tau.p + (size_t)kMfmaQueries * kHot;
    p.slots = s->d_slots.p;
    p.cand_cnt = s->d_cnt.p;
    p.cand = s->d_cand.p;
    p.cand_s = s->d_cand_s.p;
    p.cand_cap = s->cand_cap;
    p.out = s->d_hits.p;
    if (r.kind != PassRequest::kRange) {
        if (r.topk.d_out) p.out = r.topk.d_out;
        p.out_host = r.topk.download ? s->pin->hits : nullptr;
        p.flag_rec = r.topk.d_flag;
    }
    p.cnt_host = s->pin->cnt;
    p.coarse_host = s->pin->coarse;
    p.flags = src.flags;
    const uint32_t seed_parts = flags_seed_parts(s->scan_flags) ? flags_seed_parts(s->scan_flags) : kSeedParts;  // tuning
    const uint32_t seg0_blocks = r.segs[0].g->nblocks();
    p.seed_blocks = std::min<uint32_t>(std::min<uint32_t>(seed_parts, kSeedParts) * kSeedPartRows / kBlockRows, seg0_blocks);
    p.seed_shift = 0;  // the seed blocks are every 2^shift-th block of segment 0, the largest stride that fits
    while (((uint64_t)p.seed_blocks << (p.seed_shift + 1)) <= seg0_blocks && p.seed_shift < 20) ++p.seed_shift;
    p.spec = s->d_spec.p;
    p.spec_rank = 0;
    p.spec_gap = NAN;
    p.spec_spread = 0.0f;
    p.spec_base_host = s->pin->spec_base;
    p.spec_top_host = s->pin->spec_top;
    p.kth_host = s->pin->kth;
#ifdef PCV_STAMPS
    s->d_stamps.ensure(8 * 65536);
    PCV_HIP(hipMemsetAsync(s->d_stamps.p, 0, 8 * 65536 * sizeof(unsigned long long), s->ctx->stream));
    p.stamps = s->d_stamps.p;
#endif
    // |s - c| bounds of the screening scores, relative to |q||x| (DESIGN.md §screening error): an f32 FMA
    // chain in any order, and one bf16 rounding per operand on top of it
    p.eps32 = (float)(s->Dp + 16) * 1.2e-7f;
    p.eps16 = 0.0039101f + 2.0f * p.eps32;
    p.max_norm = s->max_norm;
}

// 3. What a range pass has on top: every row listed and raising nothing, the bounds, lists of range.cap entries and the pinned
// blocks range_select_kernel writes its runs to.
void fill_range_part(pcv_searcher* s, const PassRequest& r, const PassLayout& L, ScanParams& p) {
    CeilRec* listed = reinterpret_cast<CeilRec*>(s->pin_pass.p + L.off_ceil);  // lo <= s <= hi for every s: listed, raises nothing
    for (int q = 0; q < r.B; ++q) listed[q] = CeilRec{INFINITY, -1, -INFINITY, INFINITY};
    p.ceil = reinterpret_cast<const CeilRec*>(s->d_pass.p + L.off_ceil);
    std::memcpy(s->pin_pass.p + L.off_range, r.range.recs, (size_t)r.B * sizeof(RangeRec));
    p.range = reinterpret_cast<const RangeRec*>(s->d_pass.p + L.off_range);
    p.range_runs = (r.range.cap + kRangeRun - 1) / kRangeRun;
    p.range_keep = r.range.keep;
    const size_t n_cnt = (size_t)r.B * p.range_runs;
    s->pin_range.ensure(n_cnt * p.range_keep);
    s->pin_range_cnt.ensure(n_cnt);
    p.range_out = s->pin_range.p;
    p.range_cnt = s->pin_range_cnt.p;
    s->d_cand.ensure((size_t)r.B * r.range.cap);  // (never below ensure_workspace's size; the stream is idle: finish_pass waited)
    s->d_cand_s.ensure((size_t)r.B * r.range.cap);
    p.cand = s->d_cand.p;
    p.cand_s = s->d_cand_s.p;
    p.cand_cap = r.range.cap;
}

// 4. The speculative start threshold of the pass (scan.h): the int8 / MFMA scans only (their queue has the kernel that sets
// it); the j-th largest seed slot with the smallest j whose guess fails with probability < 1e-6 on rows in an order unrelated
// to the query, and the learned gap on top.  A pass of another shape than the last lets the searcher learn afresh.
struct Guess {
    int rank = 0;        // 0: none
    float gap = NAN;     // NaN: no learned part
    float spread = 0.0f;
    bool learned() const { return gap == gap; }
    bool any() const { return rank > 0 || learned(); }
};
Guess choose_guess(pcv_searcher* s, const PassRequest& r, int64_t rows, int64_t seed_rows) {
    Guess g;
    const int k = r.k();
    if (r.kind != PassRequest::kRange && (s->gap_rows != rows || s->gap_k != k || s->gap_nseg != r.nseg)) {  // another shape: learn afresh
        s->gap_rows = rows;
        s->gap_k = k;
        s->gap_nseg = r.nseg;
        s->gaps.reset();
    }
    // (no guess under a ceiling: the check at the end of the pass counts survivors, not survivors that count)
    if (r.kernel != PCV_KERNEL_MFMA || s->spec_hold || s->spec_rest != 0 || (s->scan_flags & kFlagNoGuess) || k < 2 || r.kind != PassRequest::kTopK) return g;
    if (!(s->scan_flags & kFlagNoLearnedGuess)) g.gap = s->gaps.gap();
    g.spread = (float)s->gaps.spread;
    const double ratio = (double)seed_rows / (double)std::max<int64_t>(rows, 1);  // (seed rows) / rows
    double binom = 1.0, rj = 1.0;
    for (int j = 1; j < k && ratio < 0.25; ++j) {
        binom *= (double)(k - j) / (double)j;  // C(k-1, j)
        rj *= ratio;
        if (binom * rj < 1e-6) {
            g.rank = j;
            break;
        }
    }
    return g;
}

// 5. The launch sequence, and whether it is queued plainly or replayed from a captured graph.
struct PassLaunch {
    const PassRequest& r;
    const PassLayout& L;
    int src_kind;  // what the scan streams (PassSource)
    size_t bytes;  // of the pass block to upload: parameters and tables, and the queries unless the device has them already
};
// the pass block in pinned memory: the parameters (pass_params; dp: their device mirror) and the segment table
inline SegDesc* pass_table(const pcv_searcher* s, const PassLayout& L) { return reinterpret_cast<SegDesc*>(s->pin_pass.p + L.off_seg); }
// `timed`: with the event records around the scan kernel.  Records captured into a graph do not give times on
// replay, so a replayed pass is bracketed from outside (ev[0], ev[3]) and its scan time is taken as the share of that
// total which the scan kernel had in the plain launches of the same shape.
void launch_pass(pcv_searcher* s, const PassLaunch& l, bool timed) {
    hipStream_t st = s->ctx->stream;
    const ScanParams& p = pass_params(s);
    const ScanParams* dp = reinterpret_cast<const ScanParams*>(s->d_pass.p);
    if (timed) PCV_HIP(hipEventRecord(s->ev[0], st));
    launch_upload(st, s->pin_pass.p, s->d_pass.p, l.bytes);
    if (l.r.where == PassRequest::kDevice)
        PCV_HIP(hipMemcpyAsync(s->d_pass.p + l.L.off_q, l.r.queries, (size_t)p.B * s->D * sizeof(float), hipMemcpyDeviceToDevice, st));
    launch_prep_seed(st, p, dp, pass_table(s, l.L)[0]);
    if (p.range) launch_range_thresholds(st, p, dp);
    if (timed) PCV_HIP(hipEventRecord(s->ev[1], st));
    if (l.r.kernel == PCV_KERNEL_MFMA && l.src_kind == 2)
        launch_scan_mfma8(st, p, dp, s->ctx->num_cus);
    else if (l.r.kernel == PCV_KERNEL_MFMA)
        launch_scan_mfma(st, p, dp, s->ctx->num_cus);
    else
        launch_scan_wave(st, p, dp, s->ctx->num_cus);
    if (timed) PCV_HIP(hipEventRecord(s->ev[2], st));
    if (p.range)
        launch_range_select(st, p, dp);
    else
        launch_rescore_select(st, p, dp);
    if (timed) PCV_HIP(hipEventRecord(s->ev[3], st));
}

pcv_searcher::PassShape pass_shape(const pcv_searcher* s, const PassLaunch& l, const Guess& g) {
    const ScanParams& p = pass_params(s);
    const SegDesc& seg0 = pass_table(s, l.L)[0];
    pcv_searcher::PassShape shape;
    shape.B = p.B;
    shape.k = p.k;
    shape.kernel = l.r.kernel;
    shape.src_kind = l.src_kind;
    shape.guess = p.range ? 2 : (g.any() ? 1 : 0);  // (2: a range pass, never replayed)
    shape.nseg = p.nseg;
    shape.total_blocks = p.total_blocks;
    shape.seed_blocks = p.seed_blocks;
    shape.flags = p.flags;
    shape.seg0_rows = seg0.nrows;
    shape.bytes = l.bytes;
    shape.pin = s->pin_pass.p;
    shape.dev = s->d_pass.p;
    shape.seg0_blk = seg0.blk;
    shape.seg0_scale = seg0.scale;
    return shape;
}

// Captures the launch sequence of `l` into a graph and launches that; false: capture is not possible here.
bool capture_and_launch(pcv_searcher* s, const PassLaunch& l, const pcv_searcher::PassShape& shape) {
    hipStream_t st = s->ctx->stream;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        try {
            launch_pass(s, l, false);
        } catch (...) {
            ok = false;
        }
        ok = (hipStreamEndCapture(st, &graph) == hipSuccess) && ok && graph != nullptr;
    }
    const auto drop = at_exit([&] {
        if (graph) (void)hipGraphDestroy(graph);
    });
    if (!ok || hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) return false;
    if (s->graph_exec) (void)hipGraphExecDestroy(s->graph_exec);
    s->graph_exec = exec;
    s->graph_shape = shape;
    s->graph_fixed_ms = s->shape_fixed_ms;
    PCV_HIP(hipGraphLaunch(exec, st));
    return true;
}

// Queues the pass; true: as a graph (only the pass as a whole is timed).  A shape is captured on its third sighting in a row,
// and only where queueing is a visible share of the pass (`may_replay`: up to kGraphRows rows — a longer pass is launched
// plainly and timed kernel by kernel, which is what the roofline figures are taken from — and never under ceilings, with
// device queries or for a range).
bool launch_or_replay(pcv_searcher* s, const PassLaunch& l, const pcv_searcher::PassShape& shape, bool may_replay) {
    hipStream_t st = s->ctx->stream;
    if (may_replay && s->graph_exec && shape == s->graph_shape) {
        PCV_HIP(hipEventRecord(s->ev[0], st));
        PCV_HIP(hipGraphLaunch(s->graph_exec, st));
        PCV_HIP(hipEventRecord(s->ev[3], st));
        return true;
    }
    if (may_replay && shape == s->last_shape && ++s->shape_seen >= 3 && s->shape_fixed_ms >= 0.0f) {
        PCV_HIP(hipEventRecord(s->ev[0], st));
        if (capture_and_launch(s, l, shape)) {
            PCV_HIP(hipEventRecord(s->ev[3], st));
            return true;
        }
        (void)hipGetLastError();  // capture is not possible here: stay with plain launches for good
        s->use_graph = false;
        launch_pass(s, l, true);
        return false;
    }
    if (!(shape == s->last_shape)) {
        s->last_shape = shape;
        s->shape_seen = 1;
        s->shape_fixed_ms = -1.0f;
    }
    launch_pass(s, l, true);
    return false;
}

// 6. What finish_pass needs to know of the pass.
// Bytes the scan kernel must pull from HBM per 32-row block of what it streams (0 f32 rows, 1 bf16 copies, 2 int8 copies,
// 3 the 6-bit copies; scan.h): the f32 pieces + the 32 row scales; the bf16 pieces; the int8 pieces + the block's scale; the
// 6-bit pieces + the block's four constants.
int64_t block_bytes(int Dp, int streamed) {
    const int64_t Dp8 = (Dp + 127) & ~127;
    switch (streamed) {
        case 3: return Dp8 * kBlockRows * 3 / 4 + (int64_t)sizeof(float4);
        case 2: return Dp8 * kBlockRows + (int64_t)kScale8Stride * 4;
        case 1: return (int64_t)Dp * 2 * kBlockRows;
        default: return (int64_t)Dp * 4 * kBlockRows + kBlockRows * 4;
    }
}
void book_pending(pcv_searcher* s, const PassSource& src, const ScanParams& p, const Guess& g, bool replayed) {
    pcv_searcher::Pending& pd = s->pending;
    pd.replayed = replayed;
    pd.active = true;
    pd.done = false;
    pd.B = p.B;
    pd.rows = src.rows;
    pd.src = src.src_kind;
    pd.mid = src.have_mid;
    pd.six = src.six;
    pd.range = p.range != nullptr;
    pd.cap = p.cand_cap;
    pd.int8_bytes = (int64_t)src.total_blocks * block_bytes(s->Dp, 2);
    pd.stream_bytes = (int64_t)src.total_blocks * block_bytes(s->Dp, src.six ? 3 : src.src_kind);
    pd.learned = g.learned();
    pd.guessing = g.any();
}

}  // namespace

// Queue one pass on the context stream without waiting for it: one H2D of (parameters, segment table, queries), then
// prep_seed, scan and rescore_select (range_select for a range pass), which write the results where the request says.
void enqueue_pass(pcv_searcher* s, const PassRequest& r) {
    const auto t_begin = std::chrono::steady_clock::now();
    ensure_workspace(s);
    ensure_pass_block(s, (size_t)r.nseg);
    if (!s->state_clean) launch_reset_scan_state(s->ctx->stream, s->d_tau.p, s->d_slots.p, s->d_cnt.p);
    s->state_clean = false;  // until finish_pass has seen the pass through
    const PassLayout L = pass_layout(s, (size_t)r.nseg, r.kind != PassRequest::kTopK);
    ScanParams& p = pass_params(s);
    SegDesc* tab = pass_table(s, L);
    const PassSource src = fill_segment_table(s, r, tab);
    fill_params(s, r, L, src, p);
    if (r.kind == PassRequest::kRange) fill_range_part(s, r, L, p);
    const Guess g = choose_guess(s, r, src.rows, std::min<int64_t>(tab[0].nrows, (int64_t)p.seed_blocks * kBlockRows));
    p.spec_rank = g.rank;
    p.spec_gap = g.gap;
    p.spec_spread = g.spread;

    size_t bytes = L.off_q;
    if (r.where == PassRequest::kHost) {
        std::memcpy(s->pin_pass.p + L.off_q, r.queries, (size_t)r.B * s->D * sizeof(float));
        bytes += (size_t)r.B * s->D * sizeof(float);
    }
    const PassLaunch l{r, L, src.src_kind, bytes};
    const bool may_replay = src.rows <= kGraphRows && s->use_graph && r.kind == PassRequest::kTopK && r.where != PassRequest::kDevice;
    const bool replayed = launch_or_replay(s, l, pass_shape(s, l, g), may_replay);
    book_pending(s, src, p, g, replayed);
    s->stats.host_enqueue_ms += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
}

// ---- finish_pass, step by step ----
namespace {

// What the survivor counts of a pass say (s->pin, written by the last kernel of the pass).
struct PassCounts {
    uint32_t mx = 0;            // longest list any query needed
    int64_t sum = 0, coarse = 0;
    bool guess_failed = false;  // fewer than k rows at some query's speculative threshold (scan.h)
};

void time_pass(pcv_searcher* s) {
    float ms_scan = 0, ms_total = 0;
    (void)hipEventElapsedTime(&ms_total, s->ev[0], s->ev[3]);
    if (s->pending.replayed) {
        ms_scan = ms_total * s->graph_fixed_ms;
    } else {
        (void)hipEventElapsedTime(&ms_scan, s->ev[1], s->ev[2]);
        s->shape_fixed_ms = ms_total > 0.0f ? std::min(1.0f, std::max(0.0f, ms_scan / ms_total)) : 0.0f;
    }
    s->stats.scan_ms += ms_scan;
    s->stats.total_ms += ms_total;
}

PassCounts book_pass(pcv_searcher* s) {
    const pcv_searcher::Pending& pd = s->pending;
    s->stats.scan_launches += 1;
    s->stats.rows_scanned += pd.rows;
    s->stats.bytes_algorithmic += pd.rows * (int64_t)s->D * 4;
    s->stats.bytes_streamed += pd.stream_bytes;
    s->stats.screening_copy = pd.src;
    s->stats.screen_bits = pd.src == 2 ? (pd.six ? 6 : 8) : 0;
    PassCounts c;
    for (int b = 0; b < pd.B; ++b) {
        const uint32_t cnt = s->pin->cnt[b];
        if (cnt == kSpecFailed) {  // repeat without the guess
            c.guess_failed = true;
        } else {
            c.mx = std::max(c.mx, cnt);
            c.sum += cnt;
        }
        c.coarse += s->pin->coarse[b];
        s->stats.mid_survivors += s->pin->coarse[kMfmaQueries + b];
        if (pd.six) s->stats.narrow_survivors += s->pin->coarse[2 * kMfmaQueries + b];
    }
    s->stats.coarse_survivors += c.coarse;
    s->stats.mid_copy = pd.mid ? 1 : 0;
    return c;
}

// AUTO: a corpus whose coarse screen keeps letting thousands of rows per query through gets its mid copy (built by the
// next search call, before its passes: open_search), and so does one where the survivors' f32 rows are a visible share
// of the pass's traffic (a survivor pulls every 128-byte line its 16-byte pieces lie in: 12 KB at 384-d, 24 KB at 768-d;
// measured gain of the copy: 12.5M x 384 3.5 %, 50M x 768 3.8 %, nothing at 100M x 384 where the share is 1.2 %)
constexpr int64_t kMidTrigger = 4096;  // coarse survivors per query and pass above which a pass counts as hot ...
constexpr int64_t kMidShare = 25;      // ... or whose f32 rows (32 B per feature: 16-byte pieces in 128-byte lines) come to more than 1/25 of the bytes streamed
void note_mid_trigger(pcv_searcher* s, int64_t coarse) {
    const int64_t fine_bytes = coarse * (int64_t)s->Dp * 32;
    if (s->pending.src == 2 && !s->pending.mid &&
        (coarse > kMidTrigger * (int64_t)s->pending.B || fine_bytes * kMidShare > (int64_t)s->pending.int8_bytes))
        s->mid_hot_passes += 1;
    else
        s->mid_hot_passes = 0;
}

// The pass is complete: the guess, if it had one, held, and teaches about the gap (scan.h: spec_gap).
void guess_held(pcv_searcher* s) {
    s->spec_hold = false;
    if (s->spec_rest > 0) s->spec_rest -= 1;
    if (s->spec_penalty > 0 && ++s->spec_clean >= 4096) s->spec_penalty = s->spec_clean = 0;
    if (s->pending.guessing) {
        for (int b = 0; b < s->pending.B; ++b) {
            const float d = s->pin->kth[b] - s->pin->spec_base[b];
            const float sp = s->pin->spec_top[b] - s->pin->spec_base[b];
            if (d == d && std::isfinite(d) && sp == sp && std::isfinite(sp)) s->gaps.add(d, sp);
        }
    }
    if (s->gaps.holdoff > 0) s->gaps.holdoff -= 1;
}

void guess_failed(pcv_searcher* s) {
    s->stats.speculation_reruns += 1;
    s->spec_hold = true;
    if (s->pending.learned) {  // what was learned did not hold: start over, and not before 256 passes have gone by
        s->gaps.reset();
        s->gaps.holdoff = 256;
    } else {  // the seed rows were not a fair sample for this query: no guesses for a while
        s->spec_penalty = std::min(1024, s->spec_penalty ? 2 * s->spec_penalty : 16);
        s->spec_rest = s->spec_penalty;
        s->spec_clean = 0;
    }
}

void grow_lists(pcv_searcher* s, uint32_t mx) {
    const uint64_t want = std::min<uint64_t>(list_need(mx), (uint64_t)s->pending.rows + 1024);
    s->cand_cap = (uint32_t)std::max<uint64_t>(want, s->cand_cap * 2ull);
    s->d_cand.ensure((size_t)kMfmaQueries * s->cand_cap);
    s->d_cand_s.ensure((size_t)kMfmaQueries * s->cand_cap);
}

}  // namespace

// Collect a queued pass: wait for the stream, book the statistics, and report whether a candidate list
// overflowed — nothing was lost then but the stored prefix is incomplete, so the lists are grown to what
// the pass needed and the caller repeats it (tau restarts, so the need can only be met or shrink on
// data that is not adversarially ordered; bounded by the row count).
bool finish_pass(pcv_searcher* s) {
    PCV_REQUIRE(s->pending.active, "no pass is pending");
    s->pending.active = false;
    const auto t_begin = std::chrono::steady_clock::now();
    PCV_HIP(hipStreamSynchronize(s->ctx->stream));  // also when nothing was launched: the caller's exchange may be queued
    s->stats.host_wait_ms += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    PCV_HIP(hipGetLastError());
    if (s->pending.done) return false;
#ifdef PCV_STAMPS
    if (const char* f = getenv("PCV_STAMPS_FILE")) {  // one record per pass: 65536 waves x 8 words
        std::vector<unsigned long long> h(8 * 65536);
        PCV_HIP(hipMemcpy(h.data(), s->d_stamps.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (FILE* fp = fopen(f, "ab")) {
            fwrite(h.data(), sizeof(unsigned long long), h.size(), fp);
            fclose(fp);
        }
    }
#endif
    s->state_clean = true;  // rescore_select_kernel left the scan state as a pass expects it
    time_pass(s);
    const PassCounts c = book_pass(s);
    if (s->pending.range) {
        // a fixed threshold lists many rows by design: neither AUTO's mid-copy trigger nor the learned gaps hear of it, and the
        // lists are search_range's to grow
        const bool over = c.mx > s->pending.cap;
        if (over)
            s->stats.overflow_reruns += 1;
        else
            s->stats.candidates += c.sum;
        return over;
    }
    note_mid_trigger(s, c.coarse);
    if (c.mx <= s->cand_cap && !c.guess_failed) {
        s->stats.candidates += c.sum;
        guess_held(s);
        return false;
    }
    if (c.guess_failed) {
        guess_failed(s);
        if (c.mx <= s->cand_cap) return true;
    }
    s->stats.overflow_reruns += 1;
    grow_lists(s, c.mx);
    return true;
}

// One pass, synchronously: repeated — the queries still on the device — while a candidate list overflows or a guess fails.
void run_pass(pcv_searcher* s, PassRequest r) {
    for (int attempt = 0;; ++attempt) {
        enqueue_pass(s, r);
        if (!finish_pass(s)) return;
        PCV_REQUIRE(attempt < 7, "candidate lists still overflow after %d reruns", attempt + 1);
        r.where = PassRequest::kResident;
    }
}


int pick_kernel(const pcv_searcher* s, int B) {
    const bool mfma_ok = mfma_pass_queries(s->Dp) > 0;  // the query tile must fit the LDS
    if (s->kernel == PCV_KERNEL_MFMA && !mfma_ok)
        PCV_FAIL(PCV_ERR_UNSUPPORTED, "the MFMA kernel cannot hold a %d-d query tile in LDS", s->D);
    if (s->kernel == PCV_KERNEL_WAVE || s->kernel == PCV_KERNEL_MFMA) return s->kernel;
    // with screening copies the MFMA kernel streams half the bytes of the wave kernel, whatever the batch
    if (mfma_ok && s->copies_kind != 0) return PCV_KERNEL_MFMA;
    return (B <= kMaxWaveQueries || !mfma_ok) ? PCV_KERNEL_WAVE : PCV_KERNEL_MFMA;
}

// `among_ranks`: the split must be the same on every rank of a sharded search, whatever copies each of them holds
int pass_queries(const pcv_searcher* s, int kernel, bool among_ranks) {
    if (kernel == PCV_KERNEL_WAVE) return kMaxWaveQueries;
    // every row has its int8 copy: the int8 scan's pass (256 queries up to 384-d); else what the bf16 / f32-row scans take.
    // Among ranks only if the host has said that this holds on EVERY rank (pcv_searcher_allow_wide_sharded_pass): the split of a
    // batch into passes is part of the exchange's protocol.
    if ((!among_ranks || s->wide_sharded) && s->copies_kind == 2 && s->Dp <= 1024)
        return std::min(kMfmaQueries, std::max(mfma8_pass_queries(s->Dp), mfma_pass_queries(s->Dp)));
    return mfma_pass_queries(s->Dp);
}

// The dot metric's f32 envelope (perceive_hip.h, DESIGN.md §4 "Magnitudes"): queries enter the screens unnormalised, and two of
// the quantities the scans form from them leave f32 while the canonical score is still finite.  Both are known before anything is
// queued — the query on the host, max_norm read back by the last finalize / update — so such a query is refused:
//   s_q = 127 / max|q_i| (quantize_queries_kernel) is inf below 127 / FLT_MAX = 3.73e-37: refused below 2^-120;
//   unit = |q| max_norm (both seed kernels), of which every margin is a multiple: inf beyond FLT_MAX — also whenever a single
//   product q_i x_i could pass FLT_MAX, the f32 accumulators' case; refused above 2^127.  Far below, sums of subnormal products
//   round by up to Dp * 2^-150 absolutely, which margin32 = 2 eps32 unit, a relative bound with Dp * 2^-24 unit to spare, covers
//   down to unit ~ 2^-125: refused below 2^-120 (margin32 is a subnormal from 2^-112 on; its own rounding is inside that spare).
// An all-zero query (every row scores 0) and a corpus of all-zero rows pass.  Not finite values fail no check here: such a query
// is dead in the kernels (no hits), as before.  `what`: kEnvelopeQuery leaves the unit test out — max_norm differs from rank to
// rank, and among the ranks of a sharded search only a condition all of them evaluate alike may refuse; kEnvelopeNone: the queries
// are on the device and are not looked at.
void check_dot_envelope(const pcv_searcher* s, const float* queries, int n_queries, const char* who, int what) {
    if (s->metric != PCV_METRIC_DOT || what == kEnvelopeNone) return;
    for (int q = 0; q < n_queries; ++q) {
        const float* v = queries + (size_t)q * s->D;
        double nq = 0.0;  // (a bound, not the canonical sum)
        float mx = 0.0f;
        for (int i = 0; i < s->D; ++i) {
            nq += (double)v[i] * (double)v[i];
            mx = std::max(mx, std::fabs(v[i]));
        }
        if (!(nq > 0.0) || !(nq < INFINITY)) continue;
        PCV_REQUIRE(mx >= 0x1p-120f,
                    "%s: query %d: largest |q_i| = %g is below 2^-120: the query quantisation scale s_q = 127 / max|q_i| leaves f32 "
                    "(dot metric envelope, perceive_hip.h)", who, q, (double)mx);
        if (what != kEnvelopeFull) continue;
        const double unit = std::sqrt(nq) * (double)s->max_norm;
        PCV_REQUIRE(unit == 0.0 || (unit >= 0x1p-120 && unit <= 0x1p127),
                    "%s: query %d: unit = |q| * max_norm = %g * %g is outside [2^-120, 2^127]: the screens' margins, multiples of it, "
                    "leave f32 (dot metric envelope, perceive_hip.h)", who, q, std::sqrt(nq), (double)s->max_norm);
    }
}

void check_search_args(const pcv_searcher* s, const float* queries, int n_queries, int k, const char* who, int k_max, int envelope) {
    PCV_REQUIRE(!s->dirty, "%s: rows were added or cleared without pcv_searcher_finalize", who);
    PCV_REQUIRE(queries != nullptr && n_queries > 0, "%s: no queries", who);
    PCV_REQUIRE(k > 0 && k <= k_max, "%s: num_results %d outside [1,%d]", who, k, k_max);
    check_dot_envelope(s, queries, n_queries, who, envelope);
}

// (SearchPlan: searcher_pass.h)
SearchPlan plan_search(pcv_searcher* s, const int64_t* source_ids, int n_sources, int n_queries, bool among_ranks) {
    PCV_HIP(hipSetDevice(s->ctx->device));
    SearchPlan plan;
    plan.segs = select_segments(s, source_ids, n_sources);
    plan.kernel = pick_kernel(s, n_queries);
    plan.qstep = pass_queries(s, plan.kernel, among_ranks);
    return plan;
}
// ... and what it starts with: fresh statistics and, if there are rows to search, AUTO's mid copies.  False: no selected rows —
// the answer to that is the caller's.
bool open_search(pcv_searcher* s, const SearchPlan& plan) {
    s->stats = pcv_scan_stats{};
    s->stats.kernel_used = plan.kernel;
    if (plan.segs.empty()) return false;
    maybe_build_mid_copies(s);
    return true;
}

// The ceilings of the pass that follows one whose last hits are `last` (one per query; pos < 0: that pass came back short —
// the query has all the rows there are): scan.h, CeilRec.  The band around the boundary is the fine screen's margin,
// 2 eps32 relative to |q||x| (x <= the largest row norm for the dot metric; 1 for cosine), plus the rounding of the f64 score to f32.
double query_norm(const float* q, int D) {
    double nq = 0.0;
    for (int i = 0; i < D; ++i) nq += (double)q[i] * (double)q[i];
    return std::sqrt(nq);
}

void next_ceilings(const pcv_searcher* s, const float* queries, int B, const pcv_hit_dev* last, CeilRec* out) {
    const float eps32 = (float)(s->Dp + 16) * 1.2e-7f;
    for (int q = 0; q < B; ++q) {
        CeilRec& c = out[q];
        if (last[q].pos < 0) {
            c = CeilRec{-INFINITY, INT64_MAX, -INFINITY, -INFINITY};
            continue;
        }
        const double unit = s->metric == PCV_METRIC_DOT ? query_norm(queries + (size_t)q * s->D, s->D) * (double)s->max_norm : 1.0;
        const double band = 2.5 * (double)eps32 * unit + std::fabs(last[q].score) * 2.4e-7 + 1e-37;
        c.score = last[q].score;
        c.pos = last[q].pos;
        c.lo = std::nextafterf((float)(last[q].score - band), -INFINITY);
        c.hi = std::nextafterf((float)(last[q].score + band), INFINITY);
    }
}

// A graph captured over rows that are about to move or to be freed must not replay: the next passes capture afresh.
void drop_pass_graph(pcv_searcher* s) {
    if (s->graph_exec) (void)hipGraphExecDestroy(s->graph_exec);
    s->graph_exec = nullptr;
    s->graph_shape = s->last_shape = pcv_searcher::PassShape{};
    s->shape_seen = 0;
}

}  // namespace pcv
