// searcher_store.cpp — the rows a searcher holds: the lifetime of a Segment, ingestion, finalize, the choice of the segments a
// call reads, and the derived copies of a segment.  Called by the other searcher units with s->mu held (declarations:
// searcher_internal.h); only the helper thread of the AUTO mid build runs beside that lock, on a list of its own.
#include <cstring>

#include "searcher_internal.h"

namespace pcv {

constexpr int64_t kGrowCapRows = (int64_t)1 << 22;  // spare room a new segment gets at most (6 GB at 384-d)
constexpr int64_t kMinSpareRows = 1024;             // ... and at least

// ---- the derived copies of a segment (scan.h) ----
// The screening copy (bf16, or int8 + block scales: `copied_rows`), the 6-bit copy made from the int8 one (`six_rows`) and the mid
// copy (`mid_rows`).  How they are freed, allocated, extended to the rows that have a scale and repaired after rows changed is
// said here, once: a new copy format or a new row-changing call has these functions to add to, and a miss is a screen that is no
// longer certified.
enum : unsigned { kCopyScreen = 1, kCopySix = 2, kCopyMid = 4, kCopyAll = 7 };

// (the caller has seen to it that no queued kernel reads them any more)
static void free_copies(Segment& g, unsigned which) {
    if (which & kCopyScreen) {
        if (g.blk16) (void)hipFree(g.blk16);
        if (g.blk8) (void)hipFree(g.blk8);
        if (g.scale8) (void)hipFree(g.scale8);
        g.blk16 = g.blk8 = nullptr;
        g.scale8 = nullptr;
        g.copied_rows = 0;
    }
    if (which & kCopySix) {
        if (g.blk6) (void)hipFree(g.blk6);
        if (g.scale6) (void)hipFree(g.scale6);
        g.blk6 = nullptr;
        g.scale6 = nullptr;
        g.six_rows = 0;
    }
    if (which & kCopyMid) {
        if (g.mid16) (void)hipFree(g.mid16);
        if (g.scale16) (void)hipFree(g.scale16);
        g.mid16 = nullptr;
        g.scale16 = nullptr;
        g.mid_rows = 0;
    }
}

void free_segment(Segment& g) {
    if (g.blk) (void)hipFree(g.blk);
    if (g.scale) (void)hipFree(g.scale);
    if (g.ids) (void)hipFree(g.ids);
    free_copies(g, kCopyAll);
    g = Segment();
}

namespace {
hipError_t alloc_mid(bool refuse, uint32_t cap_rows, int Dp, uint4** mid16, float** scale16) {
    return alloc_with_scales(refuse, mid16, (size_t)cap_rows * Dp * 2, scale16, (size_t)cap_rows * sizeof(float));
}

// What the mid copy of g lacks: rows [first, end) have their scale and no copy.  `scale8`: they are quantised with the int8 copy's
// block scales, which launch_mid_pack does only if that copy covers them all.
struct MidSpan {
    uint32_t first, end;
    const float* scale8;
};
MidSpan mid_span(const Segment& g) {
    return {g.mid16 ? g.mid_rows : 0u, g.scaled_rows, (g.blk8 && g.copied_rows >= g.scaled_rows) ? g.scale8 : nullptr};
}
}  // namespace
// The copy that is there catches up with the rows that have their scale.
void extend_mid(hipStream_t st, Segment& g, int D4) {
    if (!g.mid16 || g.mid_rows >= g.scaled_rows) return;
    const MidSpan m = mid_span(g);
    launch_mid_pack(st, g.blk, g.scale, m.scale8, g.mid16, g.scale16, m.first, m.end, D4);
    g.mid_rows = g.scaled_rows;
}
// ... and the 6-bit copy with the int8 copy it is derived from
void extend_six(hipStream_t st, Segment& g, int D4) {
    if (!g.blk6 || !g.blk8 || g.six_rows >= g.copied_rows) return;
    // (from the block of the first row not covered: the int8 copy re-packed that partial block with a new scale)
    launch_pack6(st, g.blk, g.scale, g.blk8, g.scale8, g.blk6, g.scale6, g.six_rows / kBlockRows, (g.copied_rows + kBlockRows - 1) / kBlockRows, D4);
    g.six_rows = g.copied_rows;
}

// The int8 blocks (and what is made from them) that hold `rows`: ascending, distinct, inside the copy.
std::vector<uint32_t> touched_blocks(const Segment& g, const std::vector<uint32_t>& rows) {
    std::vector<uint32_t> blocks;
    if (!g.blk8) return blocks;
    for (uint32_t r : rows)
        if (r < g.copied_rows) blocks.push_back(r / kBlockRows);
    std::sort(blocks.begin(), blocks.end());
    blocks.erase(std::unique(blocks.begin(), blocks.end()), blocks.end());
    return blocks;
}

// The f32 rows d_rows[0..nr) and their scales changed (a row came back from hiding, or got a new vector): the copies follow.
// bf16 pieces row by row; the WHOLE 32-row blocks d_blocks[0..nb) (touched_blocks) of the int8 copy — a finalize that appended
// rows to such a block while a row was hidden quantised it without that row, and a new row may need a smaller block scale —,
// the 6-bit copy from those int8 blocks, and a mid copy by blocks if it was quantised with the int8 block scales, by rows otherwise.
void repair_copies(pcv_searcher* s, Segment& g, const uint32_t* d_rows, uint32_t nr, const uint32_t* d_blocks, uint32_t nb) {
    hipStream_t st = s->ctx->stream;
    if (g.blk16) launch_repack16_rows(st, g.blk, g.scale, d_rows, nr, g.blk16, s->D4);
    if (g.blk8 && nb) launch_repack8_blocks(st, g.blk, g.scale, d_blocks, nb, g.blk8, g.scale8, s->D4);
    if (g.blk6 && nb) launch_repack6_blocks(st, g.blk, g.scale, g.blk8, g.scale8, d_blocks, nb, g.blk6, g.scale6, s->D4);
    if (g.mid16 && g.mid_rows > 0) {
        if (g.blk8 && g.copied_rows >= g.nrows)  // the copy is quantised with the int8 copy's block scales (launch_mid_pack)
            launch_repack_mid(st, g.blk, g.scale, g.scale8, d_blocks, nb, g.mid_rows, g.mid16, g.scale16, s->D4);
        else
            launch_repack_mid(st, g.blk, g.scale, nullptr, d_rows, nr, g.mid_rows, g.mid16, g.scale16, s->D4);
    }
}

// every row of every segment is covered by a mid copy (mids_present)
static bool mids_cover(const pcv_searcher* s) {
    for (const auto& src : s->sources)
        for (const auto& g : src.segs)
            if (g.nrows > 0 && (!g.mid16 || g.mid_rows < g.nrows)) return false;
    return true;
}

constexpr int kMidPasses = 2;  // AUTO builds the mid copy once that many passes in a row were hot (searcher_pass.cpp: note_mid_trigger)

// The AUTO build under way beside the searches, if any: `wait` for it, or only look whether it is done; done = its rows count.
void settle_mid_build(pcv_searcher* s, bool wait) {
    if (!s->mid_building) return;
    pcv_searcher::MidTask& t = *s->mid_task;
    if (!t.joined) {
        if (!wait && !t.queued.load(std::memory_order_acquire)) return;
        t.th.join();
        t.joined = true;
    }
    if (!t.failed) {
        if (wait)
            PCV_HIP(hipEventSynchronize(s->mid_done));
        else if (hipEventQuery(s->mid_done) != hipSuccess) {
            (void)hipGetLastError();  // (hipErrorNotReady)
            return;
        }
    }
    s->mid_building = false;
    if (t.failed) {  // (the helper thread has given back what it had allocated)
        s->mid_gave_way = true;
        s->mid_task.reset();
        return;
    }
    for (auto& it : t.items) {
        it.g->mid16 = it.mid16;
        it.g->scale16 = it.scale16;
        it.g->mid_rows = it.rows;
    }
    s->mid_task.reset();
    s->mids_present = mids_cover(s);
}

// Queue the build of the mid copies of every segment beside the searches (AUTO): a helper thread allocates and launches on
// the side stream, behind everything the context stream holds now.
static void start_mid_build(pcv_searcher* s) {
    settle_mid_build(s, true);
    if (!s->side) {
        PCV_HIP(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
        PCV_HIP(hipEventCreateWithFlags(&s->side_go, hipEventDisableTiming));
        PCV_HIP(hipEventCreateWithFlags(&s->mid_done, hipEventDisableTiming));
    }
    PCV_HIP(hipEventRecord(s->side_go, s->ctx->stream));
    PCV_HIP(hipStreamWaitEvent(s->side, s->side_go, 0));
    s->mid_task.reset(new pcv_searcher::MidTask());
    pcv_searcher::MidTask& t = *s->mid_task;
    for (auto& src : s->sources)
        for (auto& g : src.segs) {
            if (g.nrows == 0 || (g.mid16 && g.mid_rows >= g.scaled_rows)) continue;
            const MidSpan m = mid_span(g);
            t.items.push_back({&g, g.blk, g.scale, m.scale8, g.cap_rows, m.first, m.end, g.mid16, g.scale16, false});
        }
    const int device = s->ctx->device, D4 = s->D4, Dp = s->Dp;
    const bool fail = s->fail_copy_alloc;
    hipStream_t side = s->side;
    hipEvent_t done = s->mid_done;
    pcv_searcher::MidTask* tp = &t;
    t.th = std::thread([tp, device, D4, Dp, fail, side, done] {
        bool ok = hipSetDevice(device) == hipSuccess;
        try {
            for (auto& it : tp->items) {
                if (!ok) break;
                if (!it.mid16) {
                    ok = it.own = alloc_mid(fail, it.cap_rows, Dp, &it.mid16, &it.scale16) == hipSuccess;
                    if (!ok) break;
                }
                launch_mid_pack(side, it.blk, it.scale, it.scale8, it.mid16, it.scale16, it.first_row, it.rows, D4);
            }
            if (ok) ok = hipEventRecord(done, side) == hipSuccess;
        } catch (...) {
            ok = false;
        }
        if (!ok) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(side);
            for (auto& it : tp->items)
                if (it.own) {
                    if (it.mid16) (void)hipFree(it.mid16);
                    if (it.scale16) (void)hipFree(it.scale16);
                }
            tp->failed = true;
        }
        tp->queued.store(true, std::memory_order_release);
    });
    s->mid_building = true;  // (mids_present stays false: the passes go on without the copy until settle_mid_build sees it done)
}

void drop_mid_copies(pcv_searcher* s) {
    settle_mid_build(s, true);
    s->mids_present = false;
    for (auto& src : s->sources)
        for (auto& g : src.segs) free_copies(g, kCopyMid);
}

// The 6-bit copies (scan.h) go: they give way first when memory is short, and before a mid copy (a crowded screen gains nothing
// from them; 100M x 384 with both would not fit the device).
void drop_six_copies(pcv_searcher* s) {
    for (auto& src : s->sources)
        for (auto& g : src.segs) free_copies(g, kCopySix);
}
bool have_six_copies(const pcv_searcher* s) {
    for (const auto& src : s->sources)
        for (const auto& g : src.segs)
            if (g.blk6) return true;
    return false;
}
static size_t six_bytes_held(const pcv_searcher* s) {
    size_t n = 0;
    for (const auto& src : s->sources)
        for (const auto& g : src.segs)
            if (g.blk6) n += six_copy_bytes(g.cap_rows / kBlockRows, s->Dp) + (size_t)(g.cap_rows / kBlockRows) * sizeof(float4);
    return n;
}
// What the optional copies (mid, 6-bit) leave free of the device: rows, other searchers and models of the process, the candidate
// lists of an overflow rerun — a tenth of it, at least 4 GB.
static size_t copy_headroom(size_t total_b) { return std::max<size_t>((size_t)4 << 30, total_b / 10); }

// Mid copies (scan.h) of the rows that have their scale and no copy yet.  `must`: an allocation failure is an error
// (PCV_MID_COPY_ON); otherwise it ends the attempt for good (mid_gave_way).
void build_mid_copies(pcv_searcher* s, bool must) {
    settle_mid_build(s, true);
    hipStream_t st = s->ctx->stream;
    if (have_six_copies(s)) {
        PCV_HIP(hipStreamSynchronize(st));
        drop_six_copies(s);
    }
    for (auto& src : s->sources)
        for (auto& g : src.segs) {
            if (g.nrows == 0 || (g.mid16 && g.mid_rows >= g.scaled_rows)) continue;
            if (!g.mid16) {
                const hipError_t e = alloc_mid(s->fail_copy_alloc, g.cap_rows, s->Dp, &g.mid16, &g.scale16);
                if (e != hipSuccess) {
                    if (must)
                        PCV_FAIL(PCV_ERR_DEVICE, "hipMalloc of %.2f GB for the mid copy of %u rows failed: %s", (size_t)g.cap_rows * s->Dp * 2 / 1e9, g.cap_rows,
                                 hipGetErrorString(e));
                    PCV_HIP(hipStreamSynchronize(st));
                    drop_mid_copies(s);
                    s->mid_gave_way = true;
                    return;
                }
                g.mid_rows = 0;
            }
            extend_mid(st, g, s->D4);
        }
    s->mids_present = mids_cover(s);
}

// AUTO mid copy: called by every search entry point in front of its passes
void maybe_build_mid_copies(pcv_searcher* s) {
    settle_mid_build(s, false);
    if (!(s->mid_copy == PCV_MID_COPY_AUTO && !s->mids_present && !s->mid_building && !s->mid_gave_way && s->mid_hot_passes >= kMidPasses)) return;
    // (only if the memory is plainly there: the copy is a convenience — a few per cent of a pass on Gaussian rows, a quarter on
    // clustered ones — and the headroom is for rows, for other searchers and models of the process, for the candidate lists of
    // an overflow rerun: a tenth of the device, at least 4 GB, stays free)
    // (the 6-bit copies go before a mid copy is built — scan.h — so their bytes count as free; they are dropped only if it is)
    size_t free_b = 0, total_b = 0, need = 0;
    for (const auto& src : s->sources)
        for (const auto& g : src.segs) need += (size_t)g.cap_rows * ((size_t)s->Dp * 2 + 4);
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b + six_bytes_held(s) > need + copy_headroom(total_b)) {
        if (have_six_copies(s)) {
            PCV_HIP(hipStreamSynchronize(s->ctx->stream));
            drop_six_copies(s);
        }
        start_mid_build(s);  // beside the searches: this call and the next ones go on without it meanwhile
    } else
        s->mid_gave_way = true;
    s->mid_hot_passes = 0;
}

void drop_screening_copies(pcv_searcher* s) {
    settle_mid_build(s, true);  // (it reads the int8 copy's block scales)
    s->copies_kind = 0;
    for (auto& src : s->sources)
        for (auto& g : src.segs) free_copies(g, kCopySix | kCopyScreen);
}

// the form AUTO stands for
int copy_kind_wanted(const pcv_searcher* s) {
    if (s->screen_copy == PCV_SCREEN_COPY_OFF || s->screen_copy_gave_way) return 0;
    if (s->screen_copy == PCV_SCREEN_COPY_BF16) return 1;
    // the int8 screen goes up to 1024 padded features (scan_mfma8_kernel); AUTO keeps the bf16 form for wider rows, as
    // long as the MFMA scan can stage their query tile at all
    if (s->Dp > 1024) return (s->screen_copy == PCV_SCREEN_COPY_AUTO && mfma_pass_queries(s->Dp) > 0) ? 1 : (s->screen_copy == PCV_SCREEN_COPY_AUTO ? 0 : 2);
    return 2;
}

// What the pass chooser reads, from the segments as they are: the kind of screening copy that covers every row of every segment
// (copies_kind; 0: none does, or there are no rows), and whether the mid copies (still) do.  One rule for finalize, remove and a
// view build: a segment without rows counts for nothing, and no rows at all is no kind.  (finalize used to ask for "no source"
// instead: the same thing there, where every empty tail has just been freed and every empty source erased; a view has no
// segment without rows.)  mids_present is only ever taken back here; the mid builds raise it (mids_cover).
void refresh_copy_state(pcv_searcher* s) {
    const int kind = copy_kind_wanted(s);
    bool any = false, all = true;
    for (const auto& src : s->sources)
        for (const auto& g : src.segs) {
            if (g.nrows == 0) continue;
            any = true;
            if ((kind == 1 ? g.blk16 == nullptr : g.blk8 == nullptr) || g.copied_rows < g.nrows) all = false;
        }
    s->copies_kind = any && all ? kind : 0;
    s->mids_present = s->mids_present && mids_cover(s);
}

// hipMalloc that makes room when the device is full.  What gives way, in this order, each kind once and for good (its *_gave_way
// flag), the stream drained before it is freed: the 6-bit copies — before anything else, also to the copy they are derived
// from —; a mid copy AUTO built by itself — before the screening copies do, and to a screening copy the host asked for —; and,
// `last_rung` (for rows only), AUTO's screening copies: the f32 rows are scanned from then on.  Copies asked for explicitly stay.
static hipError_t malloc_giving_way(pcv_searcher* s, void** ptr, size_t bytes, bool last_rung) {
    hipError_t e = hipMalloc(ptr, bytes);
    auto again_without = [&](void (*drop)(pcv_searcher*), bool& gave_way) {
        (void)hipGetLastError();
        PCV_HIP(hipStreamSynchronize(s->ctx->stream));
        drop(s);
        gave_way = true;
        e = hipMalloc(ptr, bytes);
    };
    if (e != hipSuccess && have_six_copies(s)) again_without(drop_six_copies, s->six_gave_way);
    if (e != hipSuccess && s->mids_present && s->mid_copy == PCV_MID_COPY_AUTO) again_without(drop_mid_copies, s->mid_gave_way);
    if (e != hipSuccess && last_rung && s->screen_copy == PCV_SCREEN_COPY_AUTO && !s->screen_copy_gave_way)
        again_without(drop_screening_copies, s->screen_copy_gave_way);
    return e;
}

// Allocate a segment with room for `cap_rows` rows; zero-filled so padding rows / features are exact
// zeros and no row is searchable before its scale has been computed.
Segment alloc_segment(pcv_searcher* s, int64_t cap_rows, bool with_ids) {
    PCV_REQUIRE(cap_rows > 0 && cap_rows <= kMaxSegRows, "segment of %lld rows is out of range", (long long)cap_rows);
    Segment g;
    const uint32_t nblk = (uint32_t)((cap_rows + kBlockRows - 1) / kBlockRows);
    g.cap_rows = nblk * kBlockRows;
    const size_t bytes = (size_t)nblk * s->D4 * 32 * sizeof(float4);
    const hipError_t e = malloc_giving_way(s, (void**)&g.blk, bytes, true);  // the rows themselves come first
    if (e != hipSuccess) {
        (void)hipGetLastError();
        PCV_FAIL(PCV_ERR_DEVICE, "hipMalloc of %.2f GB for %lld corpus rows failed: %s", bytes / 1e9,
                 (long long)cap_rows, hipGetErrorString(e));
    }
    try {
        PCV_HIP(hipMalloc((void**)&g.scale, (size_t)g.cap_rows * sizeof(float)));
        if (with_ids) PCV_HIP(hipMalloc((void**)&g.ids, (size_t)g.cap_rows * sizeof(int64_t)));
        PCV_HIP(hipMemsetAsync(g.blk, 0, bytes, s->ctx->stream));
        PCV_HIP(hipMemsetAsync(g.scale, 0, (size_t)g.cap_rows * sizeof(float), s->ctx->stream));
        if (with_ids) PCV_HIP(hipMemsetAsync(g.ids, 0xff, (size_t)g.cap_rows * sizeof(int64_t), s->ctx->stream));
    } catch (...) {
        free_segment(g);
        throw;
    }
    return g;
}

void assign_positions(pcv_searcher* s) {
    int64_t pos = s->shard_offset;
    for (auto& src : s->sources)
        for (auto& g : src.segs) {
            g.pos0 = pos;
            pos += g.nrows;
        }
}

// Where the next `n` rows of a source go: the spare room of its last segment first, then new segments.
// A new segment is sized for what is announced (pcv_searcher_reserve) or, failing that, for as many rows
// again as the source already holds, so that a source fed by many small adds ends up in O(log n)
// segments (search.rs:138-140 sizes its per-source index from the row count the same way).
namespace {
struct Piece {
    size_t seg;  // index into src.segs
    int64_t n;
};
}  // namespace
static std::vector<Piece> place_rows(pcv_searcher* s, Source& src, int64_t n, bool with_ids) {
    settle_mid_build(s, true);
    std::vector<Piece> out;
    int64_t remaining = n;
    if (!src.segs.empty()) {
        Segment& tail = src.segs.back();
        if ((tail.ids != nullptr) == with_ids && tail.nrows < tail.cap_rows) {
            const int64_t m = std::min<int64_t>(remaining, (int64_t)tail.cap_rows - tail.nrows);
            out.push_back({src.segs.size() - 1, m});
            remaining -= m;
        }
    }
    int64_t have = src.rows() + (n - remaining);
    while (remaining > 0) {
        // room for the rows at hand plus, for later adds, as many again as the source holds by then (at least
        // kMinSpareRows, at most kGrowCapRows) — or exactly what the host announced
        const int64_t announced = std::max<int64_t>(0, src.reserve - have);
        const int64_t spare = announced > 0 ? std::max<int64_t>(0, announced - remaining)
                                            : std::min<int64_t>(std::max<int64_t>(have + remaining, kMinSpareRows), kGrowCapRows);
        int64_t cap = std::min<int64_t>(remaining + spare, kMaxSegRows);
        const int64_t need = std::min<int64_t>(remaining, kMaxSegRows);
        Segment g;
        try {
            g = alloc_segment(s, cap, with_ids);
        } catch (const Error& e) {
            if (e.status != PCV_ERR_DEVICE || cap == need) throw;
            g = alloc_segment(s, need, with_ids);  // no room for the spare rows: take exactly what is needed
        }
        src.segs.push_back(g);
        const int64_t m = std::min<int64_t>(remaining, (int64_t)g.cap_rows);
        out.push_back({src.segs.size() - 1, m});
        remaining -= m;
        have += m;
    }
    return out;
}

// build_sources row insert (search.rs:87-113,146-148): rows go to the device as they arrive — staged in
// steps of kStageRows and packed into the blocked layout — so the host never holds more than the caller's
// own buffer.  `rows` is row-major f32 or, equivalently on this little-endian host, the blob bytes.
void append_rows(pcv_searcher* s, Source& src, const int64_t* ids, const void* rows, int64_t n) {
    hipStream_t st = s->ctx->stream;
    const size_t row_bytes = (size_t)s->D * sizeof(float);
    s->dirty = true;
    int64_t done = 0;
    for (const Piece& pc : place_rows(s, src, n, true)) {
        for (int64_t off = 0; off < pc.n;) {
            Segment& g = src.segs[pc.seg];
            const int64_t m = std::min<int64_t>(kStageRows, pc.n - off);
            s->d_stage.ensure((size_t)std::min<int64_t>(kStageRows, std::max<int64_t>(m, std::min<int64_t>(n, kStageRows))) * s->D);
            PCV_HIP(hipMemcpyAsync(s->d_stage.p, (const uint8_t*)rows + (size_t)done * row_bytes, (size_t)m * row_bytes,
                                   hipMemcpyHostToDevice, st));
            launch_pack_rows(st, s->d_stage.p, m, s->D, s->D4, g.blk, g.nrows);
            if (ids)
                PCV_HIP(hipMemcpyAsync(g.ids + g.nrows, ids + done, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, st));
            else
                launch_iota_ids(st, g.ids + g.nrows, src.next_implicit_id + done, m);
            PCV_HIP(hipStreamSynchronize(st));  // the staging buffer (and the caller's memory) are free again
            g.nrows += (uint32_t)m;
            off += m;
            done += m;
        }
    }
    src.next_implicit_id += n;
}

// AUTO builds the 6-bit copy for searchers of at least kSixRows rows (PCV_SCAN_FLAGS bit 31: at any size; bit 29: never), rows of
// up to 384 features, and not beside a mid copy.
constexpr int64_t kSixRows = (int64_t)8 << 20;
static bool six_wanted(const pcv_searcher* s) {
    if (s->view_parent) return s->screen_copy == PCV_SCREEN_COPY_INT8 && have_six_copies(s->view_parent);  // a view keeps what its parent keeps
    if (s->screen_copy != PCV_SCREEN_COPY_AUTO || s->screen_copy_gave_way || s->six_gave_way || (s->scan_flags & kTuneNoSix)) return false;
    if (((s->Dp + 127) & ~127) > 384 || s->mids_present || s->mid_building || s->mid_copy == PCV_MID_COPY_ON) return false;
    if (s->scan_flags & kTuneForceSix) return true;
    int64_t rows = 0;
    for (const auto& src : s->sources) rows += src.rows();
    return rows >= kSixRows;
}

// The 6-bit copies of every segment's rows that have their int8 copy, derived from it (pack6_kernel), after the screening copies
// of every source are built: a pass streams them only if every selected segment has one.  Like the mid copy they are built only
// if the device keeps its headroom afterwards (copy_headroom), and an allocation failure or a lack of room drops them all for good
// on this searcher (six_gave_way, until rows are given back): they are a speed-up, never a requirement.
void build_six_copies(pcv_searcher* s) {
    if (!six_wanted(s)) return;
    hipStream_t st = s->ctx->stream;
    size_t need = 0;
    for (const auto& src : s->sources)
        for (const auto& g : src.segs)
            if (g.nrows > 0 && g.blk8 && !g.blk6)
                need += six_copy_bytes(g.cap_rows / kBlockRows, s->Dp) + (size_t)(g.cap_rows / kBlockRows) * sizeof(float4);
    size_t free_b = 0, total_b = 0;
    if (need > 0 && !s->fail_copy_alloc &&
        !(hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > need + copy_headroom(total_b))) {
        (void)hipGetLastError();
        PCV_HIP(hipStreamSynchronize(st));
        drop_six_copies(s);
        s->six_gave_way = true;
        return;
    }
    for (auto& src : s->sources)
        for (auto& g : src.segs) {
            if (g.nrows == 0 || !g.blk8 || (g.blk6 && g.six_rows >= g.copied_rows)) continue;
            if (!g.blk6) {
                const uint32_t nblk = g.cap_rows / kBlockRows;
                if (alloc_with_scales(s->fail_copy_alloc, &g.blk6, six_copy_bytes(nblk, s->Dp), &g.scale6, (size_t)nblk * sizeof(float4)) != hipSuccess) {
                    PCV_HIP(hipStreamSynchronize(st));
                    drop_six_copies(s);
                    s->six_gave_way = true;
                    return;
                }
                g.six_rows = 0;
            }
            extend_six(st, g, s->D4);
        }
}

// Screening copies (scan.h) of the rows that got their scale since the last finalize.  Asked for explicitly: a failed
// allocation is an error; AUTO: it switches the copies off for this searcher (the f32 rows are scanned instead).
void build_screening_copies(pcv_searcher* s, Source& src) {
    const int kind = copy_kind_wanted(s);
    if (kind == 0) return;
    if (kind == 2 && s->Dp > 1024)
        PCV_FAIL(PCV_ERR_UNSUPPORTED, "the int8 screening copy goes up to 1024 features (this index has %d): use PCV_SCREEN_COPY_BF16 or AUTO", s->D);
    hipStream_t st = s->ctx->stream;
    for (auto& g : src.segs) {
        if (g.nrows == 0) continue;
        const bool present = kind == 1 ? g.blk16 != nullptr : g.blk8 != nullptr;
        if (present && g.copied_rows >= g.scaled_rows) continue;
        if (!present) {
            free_copies(g, kCopyScreen);  // (a copy of the other kind, left from a mode change, goes first)
            const size_t nblk = g.cap_rows / kBlockRows;
            const size_t bytes = kind == 1 ? nblk * (s->D4 / 2) * 32 * sizeof(uint4) : nblk * (size_t)(((s->Dp + 127) & ~127) / 16) * 32 * sizeof(uint4);
            // (the scales are allocated behind the ladder, not with alloc_with_scales: only the copy itself makes others give way)
            hipError_t e = s->fail_copy_alloc ? hipErrorOutOfMemory  // (PCV_TUNE_FAIL_COPY_ALLOC)
                                              : malloc_giving_way(s, kind == 1 ? (void**)&g.blk16 : (void**)&g.blk8, bytes, false);
            if (e == hipSuccess && kind == 2) {
                e = hipMalloc((void**)&g.scale8, (size_t)(g.cap_rows / kBlockRows) * kScale8Stride * sizeof(float));
                if (e != hipSuccess) {
                    (void)hipFree(g.blk8);
                    g.blk8 = nullptr;
                }
            }
            if (e != hipSuccess) {
                (void)hipGetLastError();
                g.blk16 = g.blk8 = nullptr;
                g.scale8 = nullptr;
                if (s->screen_copy != PCV_SCREEN_COPY_AUTO)
                    PCV_FAIL(PCV_ERR_DEVICE, "hipMalloc of %.2f GB for the screening copy of %u rows failed: %s", bytes / 1e9, g.cap_rows,
                             hipGetErrorString(e));
                PCV_HIP(hipStreamSynchronize(st));
                drop_screening_copies(s);
                s->screen_copy_gave_way = true;
                return;
            }
        }
        if (kind == 1)
            launch_coarse_pack(st, g.blk, g.scale, g.blk16, g.copied_rows / kBlockRows, g.nblocks(), s->D4);
        else
            launch_coarse_pack8(st, g.blk, g.scale, g.blk8, g.scale8, g.copied_rows / kBlockRows, g.nblocks(), s->D4);
        g.copied_rows = g.scaled_rows;
    }
}

// The corpus bound the dot-metric screens use, as the kernels queued so far leave it (it only grows) -> s->max_norm.
void read_max_norm(pcv_searcher* s) {
    uint32_t bits = 0;
    PCV_HIP(hipMemcpyAsync(&bits, s->d_max_norm_bits, 4, hipMemcpyDeviceToHost, s->ctx->stream));
    PCV_HIP(hipStreamSynchronize(s->ctx->stream));
    PCV_HIP(hipGetLastError());
    std::memcpy(&s->max_norm, &bits, 4);
}

void do_finalize(pcv_searcher* s) {
    settle_mid_build(s, true);
    hipStream_t st = s->ctx->stream;
    IdBatch hidden;  // (the hidden set, looked up only where new rows get their scale and only if it is not empty)
    hidden.ids = &s->hidden;
    for (auto& src : s->sources) {
        for (auto& g : src.segs) {
            if (g.scaled_rows >= g.nrows) continue;
            launch_row_scales(st, g.blk, g.scaled_rows / kBlockRows, g.nblocks(), g.nrows, s->D4, s->metric, g.scale,
                              s->d_max_norm_bits);
            if (!s->hidden.empty()) {
                // row_scales_kernel starts at the block of the first new row: the hidden rows in front of it in that block lost their
                // scale 0 again (already counted); the new rows with a hidden id are hidden before any copy is made of them
                const uint32_t r0 = g.scaled_rows / kBlockRows * kBlockRows;
                hide_rows_in(s, g, r0, g.scaled_rows, hidden);
                g.hidden_rows += hide_rows_in(s, g, g.scaled_rows, g.nrows, hidden);
            }
            g.scaled_rows = g.nrows;
        }
        build_screening_copies(s, src);
        // a reserved but never filled tail is given back
        while (!src.segs.empty() && src.segs.back().nrows == 0) {
            PCV_HIP(hipStreamSynchronize(st));
            free_segment(src.segs.back());
            src.segs.pop_back();
        }
        src.reserve = 0;
    }
    // sources emptied by clear_source and never refilled disappear (rebuild_source, search.rs:67-69)
    s->sources.erase(std::remove_if(s->sources.begin(), s->sources.end(),
                                    [](const Source& x) { return x.segs.empty(); }),
                     s->sources.end());
    if (s->mid_copy == PCV_MID_COPY_ON || (s->mid_copy == PCV_MID_COPY_AUTO && s->mids_present))
        build_mid_copies(s, s->mid_copy == PCV_MID_COPY_ON);  // new rows join the copy that is there
    build_six_copies(s);  // (over every source: a pass streams them only if every selected segment has one)
    assign_positions(s);
    refresh_copy_state(s);
    read_max_norm(s);
    s->d_stage.release();
    s->dirty = false;
    s->gen += 1;  // (views copy the rows again at their next call)
}

// source_ids == NULL: every source; otherwise exactly the n_sources listed ones (search.rs:166 — an
// empty list matches nothing)
std::vector<SelSeg> select_segments(pcv_searcher* s, const int64_t* source_ids, int n_sources) {
    std::vector<SelSeg> out;
    const bool all = source_ids == nullptr;
    for (const auto& src : s->sources) {
        // rows staged for a rebuild (PCV_STAGING_SOURCE) are nobody's rows yet: "every source" does not mean them — between the
        // staging finalize and the swap an all-sources search would otherwise return the new rows beside the old ones
        bool sel = all && src.id != PCV_STAGING_SOURCE;
        for (int i = 0; i < n_sources && !sel; ++i) sel = (source_ids[i] == src.id);  // search.rs:166
        if (!sel) continue;
        for (const auto& g : src.segs)
            if (g.nrows > 0) out.push_back({&g});
    }
    return out;
}

int64_t selected_rows(const std::vector<SelSeg>& segs) {
    int64_t n = 0;
    for (const SelSeg& g : segs) n += g.g->nrows;
    return n;
}

}  // namespace pcv
