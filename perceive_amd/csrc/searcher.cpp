// searcher.cpp — host side of the Searcher C ABI (replaces search.rs:29-260 of the reference).
//
// A searcher owns, per source, a list of device-resident corpus segments in the blocked HBM layout
// (scan.h).  Searching streams the selected segments once; see scan_kernels.hip for the pipeline.
#include <dlfcn.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <memory>
#include <atomic>
#include <mutex>
#include <numeric>
#include <thread>
#include <vector>

#include "common.h"
#include "corpus.h"
#include "scan.h"
#include "searcher_internal.h"

using namespace pcv;

namespace {

constexpr int64_t kStageRows = 1 << 18;                  // rows per H2D staging step (384-d: 400 MB)
constexpr int64_t kMaxSegRows = (int64_t)0xffffffc0u;    // a candidate names its row in 32 bits
constexpr int64_t kGrowCapRows = (int64_t)1 << 22;       // spare room a new segment gets at most (6 GB at 384-d)
constexpr int64_t kMinSpareRows = 1024;                  // ... and at least
constexpr int64_t kGraphRows = (int64_t)4 << 20;        // passes over more rows than this are not replayed as graphs

// ---- the derived copies of a segment (scan.h) ----
// The screening copy (bf16, or int8 + block scales: `copied_rows`), the 6-bit copy made from the int8 one (`six_rows`) and the mid
// copy (`mid_rows`).  How they are freed, allocated, extended to the rows that have a scale and repaired after rows changed is
// said here, once: a new copy format or a new row-changing call has these functions to add to, and a miss is a screen that is no
// longer certified.
enum : unsigned { kCopyScreen = 1, kCopySix = 2, kCopyMid = 4, kCopyAll = 7 };

// (the caller has seen to it that no queued kernel reads them any more)
void free_copies(Segment& g, unsigned which) {
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
bool mids_cover(const pcv_searcher* s) {
    for (const auto& src : s->sources)
        for (const auto& g : src.segs)
            if (g.nrows > 0 && (!g.mid16 || g.mid_rows < g.nrows)) return false;
    return true;
}

constexpr int64_t kMidTrigger = 4096;  // coarse survivors per query and pass above which AUTO builds the mid copy ...
constexpr int64_t kMidShare = 25;      // ... or whose f32 rows (32 B per feature: 16-byte pieces in 128-byte lines) come to more than 1/25 of the bytes streamed ...
constexpr int kMidPasses = 2;          // ... once that many passes in a row were above it

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
void start_mid_build(pcv_searcher* s) {
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
size_t six_bytes_held(const pcv_searcher* s) {
    size_t n = 0;
    for (const auto& src : s->sources)
        for (const auto& g : src.segs)
            if (g.blk6) n += six_copy_bytes(g.cap_rows / kBlockRows, s->Dp) + (size_t)(g.cap_rows / kBlockRows) * sizeof(float4);
    return n;
}
// What the optional copies (mid, 6-bit) leave free of the device: rows, other searchers and models of the process, the candidate
// lists of an overflow rerun — a tenth of it, at least 4 GB.
size_t copy_headroom(size_t total_b) { return std::max<size_t>((size_t)4 << 30, total_b / 10); }

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
inline int copy_kind_wanted(const pcv_searcher* s) {
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
hipError_t malloc_giving_way(pcv_searcher* s, void** ptr, size_t bytes, bool last_rung) {
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
struct Piece {
    size_t seg;  // index into src.segs
    int64_t n;
};
std::vector<Piece> place_rows(pcv_searcher* s, Source& src, int64_t n, bool with_ids) {
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
bool six_wanted(const pcv_searcher* s) {
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

// ---- hidden items (pcv_searcher_hide_ids; DESIGN.md §3 "Hidden items") ----
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

void upload_id_batch(pcv_searcher* s, IdBatch& b) {
    if (b.uploaded) return;
    const std::vector<int64_t>& ids = *b.ids;
    size_t cap = 64;  // load <= 1/2: about one probe per id looked up
    while (cap < 2 * ids.size()) cap <<= 1;
    PCV_REQUIRE(cap <= ((size_t)1 << 32), "hide_ids: %zu ids in one batch", ids.size());
    std::vector<int64_t> tab(cap, kIdEmpty);
    std::vector<uint32_t> val(b.slots ? cap : 0, 0);
    b.tmask = (uint32_t)(cap - 1);
    for (size_t i = 0; i < ids.size(); ++i) {
        if (ids[i] == kIdEmpty) {
            b.has_empty = true;
            if (b.slots) b.empty_slot = (*b.slots)[i];
            continue;
        }
        uint32_t h = id_hash(ids[i], b.tmask);
        while (tab[h] != kIdEmpty) h = (h + 1) & b.tmask;
        tab[h] = ids[i];
        if (b.slots) val[h] = (*b.slots)[i];
    }
    s->d_idtab.ensure(cap);
    PCV_HIP(hipMemcpyAsync(s->d_idtab.p, tab.data(), cap * sizeof(int64_t), hipMemcpyHostToDevice, s->ctx->stream));
    if (b.slots) {
        s->d_idslot.ensure(cap);
        PCV_HIP(hipMemcpyAsync(s->d_idslot.p, val.data(), cap * sizeof(uint32_t), hipMemcpyHostToDevice, s->ctx->stream));
    }
    PCV_HIP(hipStreamSynchronize(s->ctx->stream));  // (tab and val go out of scope)
    b.uploaded = true;
}

// The part [first, second) of an ascending id list that names rows [r0, r1) of a segment with implicit ids (id0 + row).
std::pair<size_t, size_t> implicit_range(const std::vector<int64_t>& ids, const Segment& g, uint32_t r0, uint32_t r1) {
    const auto lo = std::lower_bound(ids.begin(), ids.end(), g.id0 + (int64_t)r0);
    const auto hi = std::lower_bound(lo, ids.end(), g.id0 + (int64_t)r1);
    return {(size_t)(lo - ids.begin()), (size_t)(hi - ids.begin())};
}

// The id column of rows [r0, r1) of g, streamed once against the batch's table: the matching rows -> s->d_hrows[0..n), n returned;
// with slots (match_id_slots_kernel; hide does not pay for them) each row's slot -> s->d_hslots as well, and both lists come to
// the host with the count (one round trip).
uint32_t match_id_column(pcv_searcher* s, const Segment& g, uint32_t r0, uint32_t r1, IdBatch& b, std::vector<uint32_t>* rows = nullptr,
                         std::vector<uint32_t>* slots = nullptr) {
    hipStream_t st = s->ctx->stream;
    upload_id_batch(s, b);
    s->d_hcnt.ensure(1);
    size_t want = std::min<size_t>(r1 - r0, std::max<size_t>(4096, 2 * b.ids->size()));
    for (;;) {
        s->d_hrows.ensure(want);
        if (b.slots) s->d_hslots.ensure(want);
        const uint32_t cap = (uint32_t)(b.slots ? std::min(s->d_hrows.n, s->d_hslots.n) : s->d_hrows.n);
        if (b.slots)
            launch_match_id_slots(st, g.ids, r0, r1, s->d_idtab.p, s->d_idslot.p, b.tmask, b.has_empty, b.empty_slot, s->d_hrows.p, s->d_hslots.p,
                                  s->d_hcnt.p, cap);
        else
            launch_match_ids(st, g.ids, r0, r1, s->d_idtab.p, b.tmask, b.has_empty, s->d_hrows.p, s->d_hcnt.p, cap);
        uint32_t n = 0;
        PCV_HIP(hipMemcpyAsync(&n, s->d_hcnt.p, sizeof(n), hipMemcpyDeviceToHost, st));
        if (rows) {
            rows->resize(cap);
            slots->resize(cap);
            PCV_HIP(hipMemcpyAsync(rows->data(), s->d_hrows.p, (size_t)cap * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            PCV_HIP(hipMemcpyAsync(slots->data(), s->d_hslots.p, (size_t)cap * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        PCV_HIP(hipStreamSynchronize(st));
        if (n <= cap) return n;
        want = n;  // (more rows carry these ids than the lists had room for: once more with room for all)
    }
}

// Rows [r0, r1) of segment g whose id is in the batch -> s->d_hrows[0..n), n returned.  Implicit ids (id0 + row) are found by
// arithmetic on the host; an id column is streamed once by match_ids_kernel.
uint32_t find_rows(pcv_searcher* s, const Segment& g, uint32_t r0, uint32_t r1, IdBatch& b) {
    hipStream_t st = s->ctx->stream;
    if (r0 >= r1) return 0;
    if (g.ids) return match_id_column(s, g, r0, r1, b);
    const auto in = implicit_range(*b.ids, g, r0, r1);
    std::vector<uint32_t> rows;
    for (size_t i = in.first; i < in.second; ++i) rows.push_back((uint32_t)((*b.ids)[i] - g.id0));
    if (rows.empty()) return 0;
    s->d_hrows.ensure(rows.size());
    PCV_HIP(hipMemcpyAsync(s->d_hrows.p, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    PCV_HIP(hipStreamSynchronize(st));
    return (uint32_t)rows.size();
}

void hide_found(pcv_searcher* s, Segment& g, uint32_t n) {
    launch_hide_rows(s->ctx->stream, s->d_hrows.p, n, g.scale, g.blk8, g.blk16, g.copied_rows, g.mid16 ? g.scale16 : nullptr, g.mid_rows,
                     s->D4);
}

// The rows come back: their scales, then the copies (repair_copies).
void unhide_found(pcv_searcher* s, Segment& g, uint32_t n) {
    hipStream_t st = s->ctx->stream;
    launch_restore_scales(st, g.blk, s->d_hrows.p, n, s->D4, s->metric, g.scale);
    std::vector<uint32_t> blocks;
    if (g.blk8) {
        std::vector<uint32_t> rows(n);
        PCV_HIP(hipMemcpyAsync(rows.data(), s->d_hrows.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        PCV_HIP(hipStreamSynchronize(st));
        blocks = touched_blocks(g, rows);
        if (!blocks.empty()) {
            s->d_hblocks.ensure(blocks.size());
            PCV_HIP(hipMemcpyAsync(s->d_hblocks.p, blocks.data(), blocks.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
    }
    repair_copies(s, g, s->d_hrows.p, n, s->d_hblocks.p, (uint32_t)blocks.size());
    if (g.blk8) PCV_HIP(hipStreamSynchronize(st));  // (blocks goes out of scope)
}

// Hide (or unhide) every row, in every source, whose id is in `batch` (ascending, distinct, none of it in the set yet / all of it
// in the set); the rows changed.
int64_t apply_id_batch(pcv_searcher* s, const std::vector<int64_t>& batch, bool hide) {
    if (batch.empty()) return 0;
    IdBatch b;
    b.ids = &batch;
    int64_t changed = 0;
    for (auto& src : s->sources)
        for (auto& g : src.segs) {
            const uint32_t n = find_rows(s, g, 0, g.nrows, b);
            if (n == 0) continue;
            if (hide)
                hide_found(s, g, n);
            else
                unhide_found(s, g, n);
            PCV_HIP(hipStreamSynchronize(s->ctx->stream));  // (d_hrows is the next segment's)
            g.hidden_rows = hide ? g.hidden_rows + n : g.hidden_rows - n;
            changed += n;
        }
    PCV_HIP(hipGetLastError());
    return changed;
}

// ---- updated items (pcv_searcher_update_rows; DESIGN.md §3 "Updated items") ----
constexpr uint32_t kSlotHidden = 0x80000000u;  // in a slot list: the slot's id is in the hidden set

// The rows of one segment that a call rewrites: rows[i] takes the vector of batch slot slots[i] (ascending; kSlotHidden or-ed in),
// and the blocks of the int8 copy they touch; off / boff: where the lists lie in d_urows / d_uslots and d_hblocks.
struct UpdateSeg {
    Segment* g = nullptr;
    std::vector<uint32_t> rows, slots, blocks;
    size_t off = 0, boff = 0;
};

// (slot, row) pairs of segment g for the batch.  Implicit ids (id0 + row) are found on the host; an id column is streamed once by
// match_id_slots_kernel.
std::vector<std::pair<uint32_t, uint32_t>> find_slots(pcv_searcher* s, const Segment& g, IdBatch& b) {
    std::vector<std::pair<uint32_t, uint32_t>> out;
    if (!g.ids) {
        const auto in = implicit_range(*b.ids, g, 0, g.nrows);
        for (size_t i = in.first; i < in.second; ++i) out.push_back({(*b.slots)[i], (uint32_t)((*b.ids)[i] - g.id0)});
        return out;
    }
    std::vector<uint32_t> rows, slots;
    const uint32_t cnt = match_id_column(s, g, 0, g.nrows, b, &rows, &slots);
    out.reserve(cnt);
    for (uint32_t i = 0; i < cnt; ++i) out.push_back({slots[i], rows[i]});
    return out;
}

// Every row, in every source, whose id is ids[i] takes the vector rows[i] (n rows of D f32, or their little-endian blob bytes);
// found[i] = 1 iff some row carries ids[i] (ids distinct, found zeroed).  Returns the rows rewritten.  Every row is found and every
// buffer allocated before the first row is written.
int64_t update_by_id(pcv_searcher* s, const int64_t* ids, const void* rows, int64_t n, const std::vector<uint32_t>& by_id,
                     std::vector<uint8_t>& found) {
    hipStream_t st = s->ctx->stream;
    std::vector<int64_t> sorted(n);
    for (int64_t i = 0; i < n; ++i) sorted[i] = ids[by_id[i]];
    // 1. find the rows (n < 2^31, update_call: the batch's table has room)
    IdBatch b;
    b.ids = &sorted;
    b.slots = &by_id;
    std::vector<UpdateSeg> us;
    size_t total = 0, total_blocks = 0;
    for (auto& src : s->sources)
        for (auto& g : src.segs) {
            if (g.nrows == 0) continue;
            auto pr = find_slots(s, g, b);
            if (pr.empty()) continue;
            std::sort(pr.begin(), pr.end());
            UpdateSeg u;
            u.g = &g;
            for (const auto& p : pr) {
                found[p.first] = 1;
                const bool hidden = std::binary_search(s->hidden.begin(), s->hidden.end(), ids[p.first]);
                u.rows.push_back(p.second);
                u.slots.push_back(p.first | (hidden ? kSlotHidden : 0u));
            }
            u.blocks = touched_blocks(g, u.rows);
            u.off = total;
            u.boff = total_blocks;
            total += u.rows.size();
            total_blocks += u.blocks.size();
            us.push_back(std::move(u));
        }
    if (total == 0) return 0;
    // 2. every buffer the writes need
    s->d_urows.ensure(total);
    s->d_uslots.ensure(total);
    if (total_blocks) s->d_hblocks.ensure(total_blocks);
    s->d_stage.ensure((size_t)std::min<int64_t>(n, kStageRows) * s->D);
    for (const auto& u : us) {
        PCV_HIP(hipMemcpyAsync(s->d_urows.p + u.off, u.rows.data(), u.rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        PCV_HIP(hipMemcpyAsync(s->d_uslots.p + u.off, u.slots.data(), u.slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (!u.blocks.empty())
            PCV_HIP(hipMemcpyAsync(s->d_hblocks.p + u.boff, u.blocks.data(), u.blocks.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                   st));
    }
    // 3. the rows and their scales, the batch staged in steps of kStageRows slots (steps no row takes a vector from are skipped)
    const size_t row_bytes = (size_t)s->D * sizeof(float);
    auto slot_less = [](uint32_t a, uint32_t b) { return (a & ~kSlotHidden) < b; };
    for (int64_t c0 = 0; c0 < n; c0 += kStageRows) {
        const int64_t m = std::min<int64_t>(kStageRows, n - c0);
        bool staged = false;
        for (const auto& u : us) {
            const size_t lo = std::lower_bound(u.slots.begin(), u.slots.end(), (uint32_t)c0, slot_less) - u.slots.begin();
            const size_t hi = std::lower_bound(u.slots.begin(), u.slots.end(), (uint32_t)(c0 + m), slot_less) - u.slots.begin();
            if (lo == hi) continue;
            if (!staged) {
                PCV_HIP(hipMemcpyAsync(s->d_stage.p, (const uint8_t*)rows + (size_t)c0 * row_bytes, (size_t)m * row_bytes,
                                       hipMemcpyHostToDevice, st));
                staged = true;
            }
            launch_update_rows(st, s->d_stage.p, (uint32_t)c0, s->d_urows.p + u.off + lo, s->d_uslots.p + u.off + lo, (uint32_t)(hi - lo),
                               s->D, s->D4, s->metric, u.g->blk, u.g->scale, s->d_max_norm_bits);
        }
        if (staged) PCV_HIP(hipStreamSynchronize(st));  // the staging buffer (and the caller's memory) are free again
    }
    // 4. the copies
    for (const auto& u : us) {
        const uint32_t nb = (uint32_t)u.blocks.size();
        repair_copies(s, *u.g, s->d_urows.p + u.off, (uint32_t)u.rows.size(), nb ? s->d_hblocks.p + u.boff : nullptr, nb);
    }
    // 5. the corpus bound the dot-metric screens use (it only grows: update_rows_kernel raised it for the new rows)
    uint32_t bits = 0;
    PCV_HIP(hipMemcpyAsync(&bits, s->d_max_norm_bits, 4, hipMemcpyDeviceToHost, st));
    PCV_HIP(hipStreamSynchronize(st));
    PCV_HIP(hipGetLastError());
    std::memcpy(&s->max_norm, &bits, 4);
    return (int64_t)total;
}

// ---- removed items (pcv_searcher_remove_ids; DESIGN.md §3 "Removed items") ----
// One segment that loses rows: the flags of its rows (1 = the row stays, view_mark_kernel's layout) and the tiles' offsets on the
// device, the offsets on the host as well (off[t] = rows that stay in front of tile t; off[tiles] = keep).
struct RemoveSeg {
    Source* src = nullptr;
    Segment* g = nullptr;
    DevBuf<uint32_t> flags4, tiles;
    std::vector<uint32_t> off;
    DevBuf<int64_t> new_ids;     // the id column an implicit-id segment gets (id0 + row), allocated and filled, not yet the segment's
    uint32_t keep = 0;           // rows that stay
    uint32_t first = 0;          // the first row that goes: the rows in front of it are not touched
    uint32_t hidden_gone = 0;    // rows that go and whose id is in the hidden set
};

// rows per compaction chunk: the ingest staging's step (whole tiles).  PCV_REMOVE_CHUNK_ROWS (diagnostic, read at each call)
// lowers it, so that small test corpora cross chunk boundaries.
uint32_t remove_chunk_rows() {
    int64_t rows = kStageRows;
    if (const char* f = getenv("PCV_REMOVE_CHUNK_ROWS")) rows = std::min<int64_t>(kStageRows, std::max<int64_t>(1, strtoll(f, nullptr, 0)));
    return (uint32_t)((rows + kViewTile - 1) / kViewTile * kViewTile);
}

// Every row, in every source, whose id is in `batch` (ascending, distinct, not empty) leaves the searcher; the rows behind it
// move down inside their segment.  Returns the rows removed.  Every row is found and every buffer allocated before the first
// row moves; the scratch (flags, offsets, id table, bounce buffer) is given back at the end, whatever happens: the local buffers
// by going out of scope, the searcher's own by `give_back` — both behind the catch below, which drains the stream first.
int64_t remove_by_id(pcv_searcher* s, const std::vector<int64_t>& batch) {
    hipStream_t st = s->ctx->stream;
    const int D4 = s->D4;
    std::vector<std::unique_ptr<RemoveSeg>> plan;
    DevBuf<uint32_t> total, sel;
    DevBuf<float4> b_blk;
    DevBuf<float> b_scale;
    DevBuf<int64_t> b_ids;
    const auto give_back = at_exit([s] {
        s->d_idtab.release();
        s->d_hrows.release();
        s->d_hcnt.release();
    });
    int64_t removed = 0;
    try {
        // 0. the rows that go AND are hidden, per segment (Segment::hidden_rows counts them): the ids of the batch that are in the set
        std::vector<int64_t> both;
        std::set_intersection(batch.begin(), batch.end(), s->hidden.begin(), s->hidden.end(), std::back_inserter(both));
        std::vector<std::pair<Segment*, uint32_t>> hidden_gone;
        if (!both.empty()) {
            IdBatch hb;
            hb.ids = &both;
            for (auto& src : s->sources)
                for (auto& g : src.segs)
                    if (const uint32_t n = find_rows(s, g, 0, g.nrows, hb)) hidden_gone.push_back({&g, n});
        }
        // 1. which rows stay: flags and tile offsets per segment (view_mark_kernel with the sense inverted, view_scan_kernel);
        //    an implicit-id segment (id0 + row) is intersected on the host and, if it loses a row, gets its id column first
        IdBatch b;
        b.ids = &batch;
        uint32_t longest = 0;  // the most rows any segment has behind the tile of its first removed row
        total.ensure(1);
        for (auto& src : s->sources)
            for (auto& g : src.segs) {
                if (g.nrows == 0) continue;
                auto r = std::make_unique<RemoveSeg>();
                r->src = &src;
                r->g = &g;
                if (!g.ids) {
                    const auto in = implicit_range(batch, g, 0, g.nrows);
                    if (in.first == in.second) continue;
                    if (in.second - in.first == g.nrows) {  // every row goes: no id column needed
                        r->keep = 0;
                        plan.push_back(std::move(r));
                        continue;
                    }
                }
                Segment* gp = &g;
                plan.push_back(std::move(r));  // (the plan owns what this segment holds: it is freed behind the catch's synchronise)
                RemoveSeg& rs = *plan.back();
                const int64_t* ids = g.ids;
                if (!ids) {
                    rs.new_ids.ensure(g.cap_rows);
                    PCV_HIP(hipMemsetAsync(rs.new_ids.p, 0xff, (size_t)g.cap_rows * sizeof(int64_t), st));
                    launch_iota_ids(st, rs.new_ids.p, g.id0, g.nrows);
                    ids = rs.new_ids.p;
                }
                upload_id_batch(s, b);
                const uint32_t nt = view_tiles(gp->nrows);
                rs.flags4.ensure((size_t)nt * 256);
                rs.tiles.ensure(nt);
                launch_view_select(st, ids, gp->nrows, s->d_idtab.p, b.tmask, b.has_empty, rs.flags4.p, rs.tiles.p, total.p, true);
                rs.off.resize((size_t)nt + 1);
                PCV_HIP(hipMemcpyAsync(&rs.keep, total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                PCV_HIP(hipMemcpyAsync(rs.off.data(), rs.tiles.p, (size_t)nt * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                PCV_HIP(hipStreamSynchronize(st));
                rs.off[nt] = rs.keep;
                if (rs.keep == gp->nrows) {  // nothing of this segment goes
                    plan.pop_back();
                    continue;
                }
                if (rs.keep == 0) continue;
                // the first row that goes: the first tile that is not full, then the first clear flag in it
                uint32_t t0 = 0;
                while (rs.off[t0 + 1] - rs.off[t0] == (uint32_t)kViewTile) ++t0;
                std::vector<uint32_t> f(256);
                PCV_HIP(hipMemcpyAsync(f.data(), rs.flags4.p + (size_t)t0 * 256, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                PCV_HIP(hipStreamSynchronize(st));
                uint32_t i = 0;
                while (i < (uint32_t)kViewTile && ((f[i >> 2] >> (8 * (i & 3))) & 1u)) ++i;
                rs.first = t0 * (uint32_t)kViewTile + i;
                longest = std::max(longest, gp->nrows - t0 * (uint32_t)kViewTile);
            }
        if (plan.empty()) return 0;
        // 2. every buffer the moves need: one chunk's row list and its bounce buffer (blocked like the destination, which may begin
        //    inside a block: one block more)
        const uint32_t chunk = std::min(remove_chunk_rows(), (longest + (uint32_t)kViewTile - 1) / (uint32_t)kViewTile * (uint32_t)kViewTile);
        if (chunk) {
            const size_t bb = (size_t)chunk / kBlockRows + 1;
            sel.ensure(chunk);
            b_blk.ensure(bb * D4 * 32);
            b_scale.ensure(bb * 32);
            b_ids.ensure(bb * 32);
        }
        // 3. the moves, segment by segment and chunk by chunk, ascending.  Chunk [s0, s1) of the old rows holds n rows that stay; they
        //    go to [d0, d0 + n), d0 = rows that stay in front of s0 <= s0 and d0 + n <= s1: the gather reads only [s0, s1), the
        //    store writes only in front of s1 and behind what the chunk before wrote, every later chunk reads from s1 on.
        for (auto& rp : plan) {
            RemoveSeg& r = *rp;
            Segment& g = *r.g;
            removed += g.nrows - r.keep;
            if (r.keep == 0) continue;
            int64_t* ids = r.new_ids.p ? r.new_ids.p : g.ids;
            for (uint32_t s0 = r.first / (uint32_t)kViewTile * (uint32_t)kViewTile; s0 < g.nrows; s0 += chunk) {
                const uint32_t s1 = (uint32_t)std::min<uint64_t>((uint64_t)s0 + chunk, g.nrows);
                const uint32_t tile0 = s0 / (uint32_t)kViewTile, tile1 = view_tiles(s1);
                const uint32_t d0 = r.off[tile0], n = r.off[tile1] - d0;
                const uint32_t skip = s0 < r.first ? r.first - s0 : 0;  // (the first chunk: rows in front of the first removed one stay put)
                if (n <= skip) continue;
                const uint32_t dst0 = d0 + skip, m = n - skip;
                launch_view_compact(st, r.flags4.p + (size_t)tile0 * 256, r.tiles.p + tile0, s1 - s0, sel.p, d0);
                launch_view_gather(st, g.blk + (size_t)(s0 / kBlockRows) * D4 * 32, g.scale + s0, ids + s0, 0, 0, sel.p + skip, m, D4,
                                   dst0 % kBlockRows, dst0 % kBlockRows + m, b_blk.p, b_scale.p, b_ids.p, nullptr);
                launch_compact_store(st, b_blk.p, b_scale.p, b_ids.p, D4, dst0, dst0 + m, g.blk, g.scale, ids);
            }
            // the tail: padding up to the end of the last block a fresh build would have written; no scale behind it
            const uint32_t end_new = (r.keep + kBlockRows - 1) / kBlockRows * kBlockRows, end_old = g.nblocks() * kBlockRows;
            launch_view_gather(st, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, D4, r.keep, end_new, g.blk, g.scale, ids, nullptr);
            if (end_old > end_new) PCV_HIP(hipMemsetAsync(g.scale + end_new, 0, (size_t)(end_old - end_new) * sizeof(float), st));
        }
        PCV_HIP(hipStreamSynchronize(st));
        // 4. the segments' books; the narrow copies start again at the block of the first moved row
        std::vector<Source*> touched;
        for (auto& rp : plan) {
            RemoveSeg& r = *rp;
            Segment& g = *r.g;
            for (const auto& h : hidden_gone)
                if (h.first == &g) g.hidden_rows -= std::min(g.hidden_rows, h.second);
            if (std::find(touched.begin(), touched.end(), r.src) == touched.end()) touched.push_back(r.src);
            if (r.keep == 0) {
                free_segment(g);  // (nrows 0: erased below)
                continue;
            }
            if (r.new_ids.p) g.ids = r.new_ids.hand_over();
            const uint32_t from = r.first / kBlockRows * kBlockRows;
            g.nrows = g.scaled_rows = r.keep;
            g.copied_rows = std::min(g.copied_rows, from);
            g.six_rows = std::min(g.six_rows, from);
            g.mid_rows = std::min(g.mid_rows, from);
        }
        for (Source* src : touched) {
            src->segs.erase(std::remove_if(src->segs.begin(), src->segs.end(), [](const Segment& x) { return x.blk == nullptr; }), src->segs.end());
            build_screening_copies(s, *src);
            for (auto& g : src->segs) {  // (behind the int8 copy: the 6-bit pack reads the blocks it has just re-packed)
                if (g.nrows == 0) continue;
                extend_six(st, g, D4);
                extend_mid(st, g, D4);
            }
        }
        assign_positions(s);
        PCV_HIP(hipStreamSynchronize(st));
        PCV_HIP(hipGetLastError());
    } catch (...) {
        (void)hipStreamSynchronize(st);  // (before anything queued work may still read is freed)
        throw;
    }
    return removed;
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
                uint32_t n = find_rows(s, g, r0, g.scaled_rows, hidden);
                if (n) hide_found(s, g, n);
                PCV_HIP(hipStreamSynchronize(st));
                n = find_rows(s, g, g.scaled_rows, g.nrows, hidden);
                if (n) hide_found(s, g, n);
                PCV_HIP(hipStreamSynchronize(st));
                g.hidden_rows += n;
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
    uint32_t bits = 0;
    PCV_HIP(hipMemcpyAsync(&bits, s->d_max_norm_bits, 4, hipMemcpyDeviceToHost, st));
    PCV_HIP(hipStreamSynchronize(st));
    PCV_HIP(hipGetLastError());
    std::memcpy(&s->max_norm, &bits, 4);
    s->d_stage.release();
    s->dirty = false;
    s->gen += 1;  // (views copy the rows again at their next call)
}

}  // namespace

// source_ids == NULL: every source; otherwise exactly the n_sources listed ones (search.rs:166 — an
// empty list matches nothing)
std::vector<SelSeg> pcv::select_segments(pcv_searcher* s, const int64_t* source_ids, int n_sources) {
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

int64_t pcv::selected_rows(const std::vector<SelSeg>& segs) {
    int64_t n = 0;
    for (const SelSeg& g : segs) n += g.g->nrows;
    return n;
}

namespace {

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
// the pass block in pinned memory: the parameters (dp: their device mirror) and the segment table
inline ScanParams& pass_params(const pcv_searcher* s) { return *reinterpret_cast<ScanParams*>(s->pin_pass.p); }
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

// What a list that needed `mx` entries is grown towards, before the caller's clamps (finish_pass and search_range clamp
// differently, on purpose): what the pass needed plus a quarter.
inline uint64_t list_need(uint32_t mx) { return (uint64_t)mx + mx / 4 + 1024; }

void grow_lists(pcv_searcher* s, uint32_t mx) {
    const uint64_t want = std::min<uint64_t>(list_need(mx), (uint64_t)s->pending.rows + 1024);
    s->cand_cap = (uint32_t)std::max<uint64_t>(want, s->cand_cap * 2ull);
    s->d_cand.ensure((size_t)kMfmaQueries * s->cand_cap);
    s->d_cand_s.ensure((size_t)kMfmaQueries * s->cand_cap);
}

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

bool hit_better(const pcv_hit_dev& a, const pcv_hit_dev& b) {
    if (a.score != b.score) return a.score > b.score;
    return a.pos < b.pos;
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
int pass_queries(const pcv_searcher* s, int kernel, bool among_ranks = false) {
    if (kernel == PCV_KERNEL_WAVE) return kMaxWaveQueries;
    // every row has its int8 copy: the int8 scan's pass (256 queries up to 384-d); else what the bf16 / f32-row scans take.
    // Among ranks only if the host has said that this holds on EVERY rank (pcv_searcher_allow_wide_sharded_pass): the split of a
    // batch into passes is part of the exchange's protocol.
    if ((!among_ranks || s->wide_sharded) && s->copies_kind == 2 && s->Dp <= 1024)
        return std::min(kMfmaQueries, std::max(mfma8_pass_queries(s->Dp), mfma_pass_queries(s->Dp)));
    return mfma_pass_queries(s->Dp);
}

void check_search_args(const pcv_searcher* s, const float* queries, int n_queries, int k, const char* who, int k_max = kMaxK) {
    PCV_REQUIRE(!s->dirty, "%s: rows were added or cleared without pcv_searcher_finalize", who);
    PCV_REQUIRE(queries != nullptr && n_queries > 0, "%s: no queries", who);
    PCV_REQUIRE(k > 0 && k <= k_max, "%s: num_results %d outside [1,%d]", who, k, k_max);
}

// What every search call settles before its first pass: the device, the selected segments, the kernel and how many queries one
// pass takes.  Nothing of the searcher changes here, so a refused kernel leaves what the caller has not touched itself.
struct SearchPlan {
    std::vector<SelSeg> segs;
    int kernel = 0;
    int qstep = 0;
};
SearchPlan plan_search(pcv_searcher* s, const int64_t* source_ids, int n_sources, int n_queries, bool among_ranks = false) {
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
void next_ceilings(const pcv_searcher* s, const float* queries, int B, const pcv_hit_dev* last, CeilRec* out) {
    const float eps32 = (float)(s->Dp + 16) * 1.2e-7f;
    for (int q = 0; q < B; ++q) {
        CeilRec& c = out[q];
        if (last[q].pos < 0) {
            c = CeilRec{-INFINITY, INT64_MAX, -INFINITY, -INFINITY};
            continue;
        }
        double unit = 1.0;
        if (s->metric == PCV_METRIC_DOT) {
            double nq = 0.0;
            for (int i = 0; i < s->D; ++i) nq += (double)queries[(size_t)q * s->D + i] * (double)queries[(size_t)q * s->D + i];
            unit = std::sqrt(nq) * (double)s->max_norm;
        }
        const double band = 2.5 * (double)eps32 * unit + std::fabs(last[q].score) * 2.4e-7 + 1e-37;
        c.score = last[q].score;
        c.pos = last[q].pos;
        c.lo = std::nextafterf((float)(last[q].score - band), -INFINITY);
        c.hi = std::nextafterf((float)(last[q].score + band), INFINITY);
    }
}

// Full search: any number of queries / segments; result [n_queries][k] hits on the host.
void search_hits(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                 int k, std::vector<pcv_hit_dev>& out) {
    check_search_args(s, queries, n_queries, k, "search", 1 << 24);
    const pcv_hit_dev none{NAN, -1, -1};
    out.assign((size_t)n_queries * k, none);
    s->stats = pcv_scan_stats{};  // (also when the kernel is refused)
    const SearchPlan plan = plan_search(s, source_ids, n_sources, n_queries);
    if (!open_search(s, plan)) return;
    const int qstep = plan.qstep;
    std::vector<CeilRec> ceil;
    std::vector<pcv_hit_dev> last;
    for (int q0 = 0; q0 < n_queries; q0 += qstep) {
        const int B = std::min(qstep, n_queries - q0);
        const float* qs = queries + (size_t)q0 * s->D;
        // One pass ranks up to kMaxK results.  More (search.rs:157-182 has no limit): the next kMaxK below the last hit of the
        // pass before, and so on — each pass exact among the rows that rank after its ceiling (the statistics add up over the passes).
        for (int got = 0; got < k; got += kMaxK) {
            const int kk = std::min(kMaxK, k - got);
            if (got > 0) {
                ceil.resize((size_t)B);
                next_ceilings(s, qs, B, last.data(), ceil.data());
            }
            run_pass(s, PassRequest(qs, B, plan.segs, plan.kernel).top_k(kk, nullptr, true, nullptr, got > 0 ? ceil.data() : nullptr));
            last.resize((size_t)B);
            bool more = false;
            for (int q = 0; q < B; ++q) {  // (the hits came down with the pass)
                std::memcpy(out.data() + (size_t)(q0 + q) * k + got, s->pin->hits + (size_t)q * kk, (size_t)kk * sizeof(pcv_hit_dev));
                last[(size_t)q] = s->pin->hits[(size_t)q * kk + kk - 1];  // pos < 0: fewer than kk rows counted — nothing is left
                more = more || last[(size_t)q].pos >= 0;
            }
            if (!more) break;
        }
    }
}

// hits -> the reference's result convention
void hits_to_outputs(int metric, int D, const pcv_hit_dev* hits, int n_queries, int k, int64_t* out_ids,
                     float* out_scores, int* out_counts) {
    for (int q = 0; q < n_queries; ++q) {
        int cnt = 0;
        for (int j = 0; j < k; ++j) {
            const pcv_hit_dev& h = hits[(size_t)q * k + j];
            const bool ok = h.pos >= 0;
            if (ok) ++cnt;
            if (out_ids) out_ids[(size_t)q * k + j] = ok ? h.id : -1;
            if (out_scores) {
                out_scores[(size_t)q * k + j] = ok ? reported_score(metric, D, h.score) : NAN;
            }
        }
        if (out_counts) out_counts[q] = cnt;
    }
}

// ---- range search (pcv_searcher_search_range; DESIGN.md §4 "Range search") ----
// The threshold of a range pass for one query: the canonical value of the bound, rounded towards "keeps more" — no row whose
// REPORTED score passes the bound has c < tau (scan.h, RangeRec).
//   cosine: (float)c >= b implies c > the f32 below b;
//   dot:    (float)max(0, 1 - c/D) <= b implies 1 - c/D < the f32 above b, i.e. c > D (1 - that), less the roundings of the f64
//           expression (1e-9 relative is generous); a negative bound admits nothing.
// Capped at a value no score reaches (cosine: 4; dot: 2 |q| max|x|), so that "nothing" is a finite threshold like any other.
RangeRec range_rec(const pcv_searcher* s, const float* q, float bound) {
    RangeRec r{bound, -INFINITY};
    float most = 4.0f;
    if (s->metric == PCV_METRIC_DOT) {
        double nq = 0.0;
        for (int i = 0; i < s->D; ++i) nq += (double)q[i] * (double)q[i];
        const double m = 2.0 * std::sqrt(nq) * (double)s->max_norm + 1e-30;
        most = (m < (double)FLT_MAX) ? std::nextafterf((float)m, INFINITY) : FLT_MAX;  // (NaN: FLT_MAX)
        if (bound < 0.0f) {
            r.tau = most;
        } else if (bound < INFINITY) {
            const double T = (double)s->D * (1.0 - (double)std::nextafterf(bound, INFINITY));
            const double Tl = T - std::fabs(T) * 1e-9;
            r.tau = Tl > -(double)FLT_MAX ? std::nextafterf((float)Tl, -INFINITY) : -INFINITY;
        }
    } else if (bound > -INFINITY) {
        r.tau = std::nextafterf(bound, -INFINITY);
    }
    if (r.tau > most) r.tau = most;
    return r;
}

// What a range call leaves allocated for the next one.  Its lists and result blocks are sized from the data: up to kRangeBudget
// list entries per pass (0.4 GB of device lists) and, with max_results >= kRangeRun, as many pcv_hit_dev of pinned host memory
// (0.8 GB).  A searcher that once answered a wide bound does not hold that for good: whatever exceeds kRangeKeptBytes is given
// back when the call ends, and the lists start from cand_cap again (at the price of one repeated pass for the next wide bound).
constexpr size_t kRangeKeptBytes = (size_t)64 << 20;
void trim_range_memory(pcv_searcher* s) {
    const bool pinned = s->pin_range.n * sizeof(pcv_hit_dev) > kRangeKeptBytes;
    const bool lists = s->d_cand.n * sizeof(*s->d_cand.p) > kRangeKeptBytes && s->d_cand.n > (size_t)kMfmaQueries * s->cand_cap;
    if (!pinned && !lists) return;
    (void)hipStreamSynchronize(s->ctx->stream);  // (a call that failed may have left its pass in flight)
    if (pinned) s->pin_range.release();
    if (lists) {  // (every pass sizes them again: ensure_workspace, fill_range_part)
        s->d_cand.release();
        s->d_cand_s.release();
        s->range_cap = 0;
    }
}

// Every searchable row of the selected sources whose reported score passes the query's bound, in the canonical order, at most
// max_results per query.  One pass per group of queries (a second one if a list was too short: the thresholds are fixed, so the
// uncapped counts of the first are exactly what the second needs); range_select_kernel leaves each list as sorted runs of
// kRangeRun in pinned memory, merged here.
void search_range(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources, const float* bounds,
                  int64_t max_results, int64_t* out_ids, float* out_scores, int64_t* out_counts, uint8_t* out_more) {
    PCV_REQUIRE(!s->dirty, "search_range: rows were added or cleared without pcv_searcher_finalize");
    s->stats = pcv_scan_stats{};  // (also when the kernel is refused)
    const SearchPlan plan = plan_search(s, source_ids, n_sources, n_queries);
    for (int q = 0; q < n_queries; ++q) {
        if (out_counts) out_counts[q] = 0;
        if (out_more) out_more[q] = 0;
    }
    auto blank = [&](int q, int64_t from) {
        for (int64_t j = from; j < max_results; ++j) {
            if (out_ids) out_ids[(size_t)q * max_results + j] = -1;
            if (out_scores) out_scores[(size_t)q * max_results + j] = NAN;
        }
    };
    if (!open_search(s, plan)) {
        for (int q = 0; q < n_queries; ++q) blank(q, 0);
        return;
    }
    struct Trim {
        pcv_searcher* s;
        ~Trim() { trim_range_memory(s); }
    } trim{s};
    std::vector<RangeRec> recs((size_t)n_queries);
    for (int q = 0; q < n_queries; ++q) recs[(size_t)q] = range_rec(s, queries + (size_t)q * s->D, bounds[q]);
    // the lists of one pass hold at most kRangeBudget entries (12 bytes each): long lists take fewer queries per pass
    constexpr uint64_t kRangeBudget = (uint64_t)1 << 25;
    const uint32_t keep = (uint32_t)std::min<int64_t>(kRangeRun, max_results);
    uint32_t cap = std::max(s->range_cap, s->cand_cap);
    const int qmost = plan.qstep;
    struct Head {
        const pcv_hit_dev* at;
        const pcv_hit_dev* end;
    };
    std::vector<Head> heads;
    for (int q0 = 0; q0 < n_queries;) {
        int B = (int)std::min<uint64_t>((uint64_t)std::min(qmost, n_queries - q0), std::max<uint64_t>(1, kRangeBudget / cap));
        const float* qs = queries + (size_t)q0 * s->D;
        PassRequest pass = PassRequest(qs, B, plan.segs, plan.kernel).in_range(recs.data() + q0, cap, keep);
        enqueue_pass(s, pass);
        if (finish_pass(s)) {
            uint32_t mx = 0;
            int worst = 0;
            for (int q = 0; q < B; ++q)
                if (s->pin->cnt[q] > mx) mx = s->pin->cnt[q], worst = q0 + q;
            if (mx > (uint32_t)PCV_MAX_RANGE_ROWS)
                PCV_FAIL(PCV_ERR_UNSUPPORTED,
                         "search_range: the pass of query %d lists %u rows, more than PCV_MAX_RANGE_ROWS (%d): use pcv_searcher_search for "
                         "such a bound",
                         worst, mx, (int)PCV_MAX_RANGE_ROWS);
            // what the pass needed plus a quarter, at least twice what they were
            const uint64_t want = std::max<uint64_t>(list_need(mx), (uint64_t)cap * 2);
            cap = (uint32_t)std::max<uint64_t>(mx, std::min<uint64_t>(want, (uint64_t)PCV_MAX_RANGE_ROWS));
            s->range_cap = cap;
            B = (int)std::min<uint64_t>((uint64_t)B, std::max<uint64_t>(1, kRangeBudget / cap));
            pass.B = B;
            pass.range.cap = cap;
            enqueue_pass(s, pass);
            PCV_REQUIRE(!finish_pass(s), "search_range: lists sized from the counts of a pass overflowed in its repeat");
        }
        const uint32_t runs = (cap + kRangeRun - 1) / kRangeRun;
        for (int q = 0; q < B; ++q) {
            const uint32_t listed = std::min(s->pin->cnt[q], cap);
            const uint32_t used = (listed + kRangeRun - 1) / kRangeRun;
            int64_t total = 0;
            heads.clear();
            for (uint32_t r = 0; r < used; ++r) {
                const uint32_t n = s->pin_range_cnt.p[(size_t)q * runs + r];
                total += n;
                const pcv_hit_dev* at = s->pin_range.p + ((size_t)q * runs + r) * keep;
                if (n > 0) heads.push_back({at, at + std::min(n, keep)});
            }
            const int64_t cnt = std::min(total, max_results);
            const size_t o = (size_t)(q0 + q) * (size_t)max_results;
            auto after = [](const Head& a, const Head& b) { return hit_better(*b.at, *a.at); };  // (heap: the best run on top)
            std::make_heap(heads.begin(), heads.end(), after);
            for (int64_t j = 0; j < cnt; ++j) {
                std::pop_heap(heads.begin(), heads.end(), after);
                Head& h = heads.back();
                if (out_ids) out_ids[o + j] = h.at->id;
                if (out_scores) out_scores[o + j] = reported_score(s->metric, s->D, h.at->score);
                if (++h.at == h.end)
                    heads.pop_back();
                else
                    std::push_heap(heads.begin(), heads.end(), after);
            }
            blank(q0 + q, cnt);
            if (out_counts) out_counts[q0 + q] = cnt;
            if (out_more) out_more[q0 + q] = total > max_results ? 1 : 0;
        }
        q0 += B;
    }
}

// ---- distinct results (pcv_searcher_search_distinct; DESIGN.md §4 "Distinct results") ----
// The state block of one group of up to kMfmaQueries queries (scan.h, DistinctArgs), the same layout on both sides.
struct DistinctLayout {
    static constexpr size_t Q = kMfmaQueries;
    static constexpr size_t off_rec = 0;
    static constexpr size_t off_kept = off_rec + Q * sizeof(DistinctRec);
    static constexpr size_t off_sim = off_kept + Q * kMaxK * sizeof(pcv_hit_dev);
    static constexpr size_t off_norm = off_sim + Q * kMaxK * sizeof(int32_t);  // (the device's alone: never downloaded)
    static constexpr size_t total = off_norm + Q * kMaxK * sizeof(double);
};

// The walk of one group of B queries, shared by the calls that collapse a ranked list (search_distinct, search_grouped): passes of
// kMaxK hits until every query is finished or `pool` entries are walked, `select` (the call's select step, queued on the stream
// after each pass) keeping the records `rec` (pinned; `d_rec` on the device) up to date.  -> per query, whether its walk stopped
// at `pool` unfinished with more of its list to come (decided only if `want_more`).
template <class Select>
std::vector<uint8_t> walk_ranked_lists(pcv_searcher* s, const SearchPlan& plan, const float* qs, int B, int pool, DistinctRec* rec,
                                       DistinctRec* d_rec, bool want_more, Select select) {
    hipStream_t st = s->ctx->stream;
    std::vector<CeilRec> ceil;
    for (int q = 0; q < B; ++q) rec[q] = DistinctRec{0, 0, 0, 0, INFINITY, -1};
    PCV_HIP(hipMemcpyAsync(d_rec, rec, (size_t)B * sizeof(DistinctRec), hipMemcpyHostToDevice, st));
    // A query still walking after a pass has walked every hit of every pass so far: `walked` is the same for all of them.
    bool pending = true;
    for (int walked = 0; pending && walked < pool; walked += kMaxK) {
        const int kk = std::min(kMaxK, pool - walked);
        if (walked > 0) {
            ceil.resize((size_t)B);
            std::vector<pcv_hit_dev> last((size_t)B);
            for (int q = 0; q < B; ++q) last[(size_t)q] = rec[q].flags ? pcv_hit_dev{NAN, -1, -1} : pcv_hit_dev{rec[q].last_score, rec[q].last_pos, -1};
            next_ceilings(s, qs, B, last.data(), ceil.data());
        }
        run_pass(s, PassRequest(qs, B, plan.segs, plan.kernel).top_k(kk, nullptr, false, nullptr, walked > 0 ? ceil.data() : nullptr));
        // (the pass block is the pass's to allocate and to grow: its device address is read after the pass, never before)
        select();
        PCV_HIP(hipStreamSynchronize(st));
        PCV_HIP(hipGetLastError());
        pending = false;
        for (int q = 0; q < B; ++q) pending = pending || rec[q].flags == 0;
    }
    // out_more: a walk that stopped at `pool` without its num_results and without seeing its list end.  Whether the list had
    // another row is one more, short pass under the same kind of ceiling: one hit per query.
    std::vector<uint8_t> more((size_t)B, 0);
    if (pending && want_more) {
        ceil.resize((size_t)B);
        std::vector<pcv_hit_dev> last((size_t)B);
        for (int q = 0; q < B; ++q) last[(size_t)q] = rec[q].flags ? pcv_hit_dev{NAN, -1, -1} : pcv_hit_dev{rec[q].last_score, rec[q].last_pos, -1};
        next_ceilings(s, qs, B, last.data(), ceil.data());
        run_pass(s, PassRequest(qs, B, plan.segs, plan.kernel).top_k(1, nullptr, true, nullptr, ceil.data()));
        for (int q = 0; q < B; ++q) more[(size_t)q] = (rec[q].flags == 0 && s->pin->hits[q].pos >= 0) ? 1 : 0;
    }
    return more;
}

// The ranked list of every query is walked kMaxK hits a pass: the first pass is a plain top-k pass, every later one ranks the rows
// behind the last hit walked (its ceiling, as in search_hits), and after each the select step (distinct_kernels.hip) walks the
// pass's lists on the device against the rows kept so far.  What comes back after a pass is one record per query — kept, examined,
// finished or not, the last hit walked —; the kept rows and their counters come down once, at the end.  A query that is finished
// (num_results kept, or its list at an end) gets the ceiling "nothing ranks after it" and the select step leaves it alone.
void search_distinct(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources, int k, float threshold,
                     int pool, int64_t* out_ids, float* out_scores, int32_t* out_counts, int32_t* out_similar, int32_t* out_examined,
                     uint8_t* out_more) {
    check_search_args(s, queries, n_queries, k, "search_distinct");
    s->stats = pcv_scan_stats{};  // (also when the kernel is refused)
    const SearchPlan plan = plan_search(s, source_ids, n_sources, n_queries);
    auto blank = [&](int q, int from) {
        for (int j = from; j < k; ++j) {
            if (out_ids) out_ids[(size_t)q * k + j] = -1;
            if (out_scores) out_scores[(size_t)q * k + j] = NAN;
            if (out_similar) out_similar[(size_t)q * k + j] = 0;
        }
    };
    if (!open_search(s, plan)) {
        for (int q = 0; q < n_queries; ++q) {
            blank(q, 0);
            if (out_counts) out_counts[q] = 0;
            if (out_examined) out_examined[q] = 0;
            if (out_more) out_more[q] = 0;
        }
        return;
    }
    using L = DistinctLayout;
    hipStream_t st = s->ctx->stream;
    s->d_distinct.ensure(L::total);
    s->pin_distinct.ensure(L::off_norm);
    DistinctRec* rec = reinterpret_cast<DistinctRec*>(s->pin_distinct.p + L::off_rec);
    DistinctArgs args{};
    args.rec = reinterpret_cast<DistinctRec*>(s->d_distinct.p + L::off_rec);
    args.rec_host = rec;
    args.kept = reinterpret_cast<pcv_hit_dev*>(s->d_distinct.p + L::off_kept);
    args.similar = reinterpret_cast<int32_t*>(s->d_distinct.p + L::off_sim);
    args.kept_norm = reinterpret_cast<double*>(s->d_distinct.p + L::off_norm);
    args.num_results = k;
    args.threshold = (double)threshold;
    const pcv_hit_dev* kept = reinterpret_cast<const pcv_hit_dev*>(s->pin_distinct.p + L::off_kept);
    const int32_t* similar = reinterpret_cast<const int32_t*>(s->pin_distinct.p + L::off_sim);
    for (int q0 = 0; q0 < n_queries; q0 += plan.qstep) {
        const int B = std::min(plan.qstep, n_queries - q0);
        const float* qs = queries + (size_t)q0 * s->D;
        const std::vector<uint8_t> more = walk_ranked_lists(s, plan, qs, B, pool, rec, args.rec, out_more != nullptr, [&] {
            launch_distinct_select(st, pass_params(s), reinterpret_cast<const ScanParams*>(s->d_pass.p), args);
        });
        PCV_HIP(hipMemcpyAsync(s->pin_distinct.p + L::off_kept, s->d_distinct.p + L::off_kept, L::off_norm - L::off_kept, hipMemcpyDeviceToHost, st));
        PCV_HIP(hipStreamSynchronize(st));
        for (int q = 0; q < B; ++q) {
            const int n = (int)rec[q].kept;
            const size_t o = (size_t)(q0 + q) * k;
            for (int j = 0; j < n; ++j) {
                const pcv_hit_dev& h = kept[(size_t)q * kMaxK + j];
                if (out_ids) out_ids[o + j] = h.id;
                if (out_scores) out_scores[o + j] = reported_score(s->metric, s->D, h.score);
                if (out_similar) out_similar[o + j] = similar[(size_t)q * kMaxK + j];
            }
            blank(q0 + q, n);
            if (out_counts) out_counts[q0 + q] = n;
            if (out_examined) out_examined[q0 + q] = (int32_t)rec[q].examined;
            if (out_more) out_more[q0 + q] = more[(size_t)q];
        }
    }
}

// ---- diverse results (pcv_searcher_search_diverse; DESIGN.md §4 "Diverse results") ----
// The state block of one group of up to kMfmaQueries queries: the walk's records and the result block, the same layout on both
// sides.  (The pool lists and the row scratch are sized by the call and live beside it: scan.h, DiverseArgs.)
struct DiverseLayout {
    static constexpr size_t Q = kMfmaQueries;
    static constexpr size_t off_rec = 0;
    static constexpr size_t off_id = off_rec + Q * sizeof(DistinctRec);
    static constexpr size_t off_score = off_id + Q * kMaxK * sizeof(int64_t);
    static constexpr size_t off_marginal = off_score + Q * kMaxK * sizeof(double);
    static constexpr size_t off_rank = off_marginal + Q * kMaxK * sizeof(double);
    static constexpr size_t off_exact = off_rank + Q * kMaxK * sizeof(int32_t);
    static constexpr size_t total = off_exact + Q * sizeof(uint32_t);
};
// The rows of a group's pools are gathered into one compact scratch of at most kDiverseScratchBytes: a group is as many queries
// as fit (64 at 384-d and the largest pool), one at least.  What exceeds kDiverseKeptBytes is given back when the call ends.
constexpr size_t kDiverseScratchBytes = (size_t)512 << 20;
constexpr size_t kDiverseKeptBytes = (size_t)64 << 20;

// The first `pool` entries of every query's ranked list are collected kMaxK hits a pass (walk_ranked_lists: nothing stops a query
// early but the end of its list), diverse_collect_kernel appending each pass's hits and their rows to the query's pool; then one
// launch of diverse_select_kernel makes the greedy walk of the whole group.  What comes back is one record per query after each
// pass and the result block once.
void search_diverse(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources, int k, float lambda,
                    int pool, int64_t* out_ids, float* out_scores, double* out_marginal, int32_t* out_ranks, int32_t* out_counts,
                    int32_t* out_examined, uint8_t* out_exact) {
    check_search_args(s, queries, n_queries, k, "search_diverse");
    s->stats = pcv_scan_stats{};  // (also when the kernel is refused)
    const SearchPlan plan = plan_search(s, source_ids, n_sources, n_queries);
    auto blank = [&](int q, int from) {
        for (int j = from; j < k; ++j) {
            if (out_ids) out_ids[(size_t)q * k + j] = -1;
            if (out_scores) out_scores[(size_t)q * k + j] = NAN;
            if (out_marginal) out_marginal[(size_t)q * k + j] = NAN;
            if (out_ranks) out_ranks[(size_t)q * k + j] = -1;
        }
    };
    if (!open_search(s, plan)) {
        for (int q = 0; q < n_queries; ++q) {
            blank(q, 0);
            if (out_counts) out_counts[q] = 0;
            if (out_examined) out_examined[q] = 0;
            if (out_exact) out_exact[q] = 1;  // (the list ended inside the pool)
        }
        return;
    }
    using L = DiverseLayout;
    hipStream_t st = s->ctx->stream;
    const size_t cap = ((size_t)pool + 63) / 64 * 64;
    const size_t row_bytes = cap * (size_t)s->D4 * sizeof(float4);  // of one query's pool
    const int group = (int)std::min<size_t>((size_t)std::min(plan.qstep, n_queries), std::max<size_t>(1, kDiverseScratchBytes / row_bytes));
    const auto trim = at_exit([&] {
        if (s->d_diverse_rows.n * sizeof(float4) <= kDiverseKeptBytes) return;
        (void)hipStreamSynchronize(st);  // (a call that failed may have left its kernels in flight)
        s->d_diverse_rows.release();
    });
    s->d_diverse.ensure(L::total);
    s->pin_diverse.ensure(L::total);
    s->d_diverse_entries.ensure((size_t)group * cap);
    s->d_diverse_rows.ensure((size_t)group * cap * (size_t)s->D4);
    DistinctRec* rec = reinterpret_cast<DistinctRec*>(s->pin_diverse.p + L::off_rec);
    DiverseArgs args{};
    args.rec = reinterpret_cast<DistinctRec*>(s->d_diverse.p + L::off_rec);
    args.rec_host = rec;
    args.entries = s->d_diverse_entries.p;
    args.rows = s->d_diverse_rows.p;
    args.out_id = reinterpret_cast<int64_t*>(s->d_diverse.p + L::off_id);
    args.out_score = reinterpret_cast<double*>(s->d_diverse.p + L::off_score);
    args.out_marginal = reinterpret_cast<double*>(s->d_diverse.p + L::off_marginal);
    args.out_rank = reinterpret_cast<int32_t*>(s->d_diverse.p + L::off_rank);
    args.out_exact = reinterpret_cast<uint32_t*>(s->d_diverse.p + L::off_exact);
    args.cap = (int)cap;
    args.pool = pool;
    args.num_results = k;
    args.lambda = (double)lambda;
    const int64_t* r_id = reinterpret_cast<const int64_t*>(s->pin_diverse.p + L::off_id);
    const double* r_score = reinterpret_cast<const double*>(s->pin_diverse.p + L::off_score);
    const double* r_marginal = reinterpret_cast<const double*>(s->pin_diverse.p + L::off_marginal);
    const int32_t* r_rank = reinterpret_cast<const int32_t*>(s->pin_diverse.p + L::off_rank);
    const uint32_t* r_exact = reinterpret_cast<const uint32_t*>(s->pin_diverse.p + L::off_exact);
    for (int q0 = 0; q0 < n_queries; q0 += group) {
        const int B = std::min(group, n_queries - q0);
        const float* qs = queries + (size_t)q0 * s->D;
        args.walked = 0;
        walk_ranked_lists(s, plan, qs, B, pool, rec, args.rec, false, [&] {
            launch_diverse_collect(st, pass_params(s), reinterpret_cast<const ScanParams*>(s->d_pass.p), args);
            args.walked += kMaxK;
        });
        launch_diverse_select(st, B, s->D, s->D4, s->metric, args);
        PCV_HIP(hipMemcpyAsync(s->pin_diverse.p + L::off_id, s->d_diverse.p + L::off_id, L::total - L::off_id, hipMemcpyDeviceToHost, st));
        PCV_HIP(hipStreamSynchronize(st));
        PCV_HIP(hipGetLastError());
        for (int q = 0; q < B; ++q) {
            const int n = (int)rec[q].kept;
            const size_t o = (size_t)(q0 + q) * k;
            for (int j = 0; j < n; ++j) {
                const size_t i = (size_t)q * kMaxK + j;
                if (out_ids) out_ids[o + j] = r_id[i];
                if (out_scores) out_scores[o + j] = reported_score(s->metric, s->D, r_score[i]);
                if (out_marginal) out_marginal[o + j] = r_marginal[i];
                if (out_ranks) out_ranks[o + j] = r_rank[i];
            }
            blank(q0 + q, n);
            if (out_counts) out_counts[q0 + q] = n;
            if (out_examined) out_examined[q0 + q] = (int32_t)rec[q].examined;
            if (out_exact) out_exact[q0 + q] = r_exact[q] ? 1 : 0;
        }
    }
}

// ---- grouped results (pcv_searcher_set_groups / _search_grouped; DESIGN.md §4 "Grouped results") ----
constexpr int64_t kMaxGroupEntries = (int64_t)1 << 30;
constexpr uint64_t kMinGroupSlots = 1024;
constexpr size_t kGroupKeptBytes = (size_t)64 << 20;  // scratch of a set_groups / get_groups call beyond this is given back

// The table of `s` gets `slots` slots (a power of two, more than it has): the entries move by a rehash on the device.  If the
// allocation fails the old table stays as it is.
void grow_groups(pcv_searcher* s, uint64_t slots) {
    pcv_searcher::Groups& t = s->groups;
    hipStream_t st = s->ctx->stream;
    int64_t *keys = nullptr, *vals = nullptr;
    const hipError_t e = alloc_with_scales(s->fail_copy_alloc, &keys, slots * sizeof(int64_t), &vals, slots * sizeof(int64_t));
    if (e != hipSuccess)
        PCV_FAIL(PCV_ERR_DEVICE, "set_groups: hipMalloc of %.2f GB for a group table of %llu slots failed: %s (the table is unchanged)",
                 slots * 16 / 1e9, (unsigned long long)slots, hipGetErrorString(e));
    try {
        launch_group_fill(st, keys, vals, slots);
        launch_group_rehash(st, t.keys, t.vals, t.slots, keys, vals, (uint32_t)(slots - 1));
        PCV_HIP(hipStreamSynchronize(st));
    } catch (...) {
        (void)hipFree(keys);
        (void)hipFree(vals);
        throw;
    }
    if (t.keys) (void)hipFree(t.keys);
    if (t.vals) (void)hipFree(t.vals);
    if (t.slots > 0) t.rehashes += 1;
    t.keys = keys;
    t.vals = vals;
    t.slots = slots;
}

void trim_group_scratch(pcv_searcher* s) {
    pcv_searcher::Groups& t = s->groups;
    if (t.d_claim.n * sizeof(uint32_t) > kGroupKeptBytes) t.d_claim.release();
    if (t.d_slot.n * sizeof(uint32_t) > kGroupKeptBytes) t.d_slot.release();
    if (t.d_batch.n * sizeof(int64_t) > kGroupKeptBytes) t.d_batch.release();
}

// The upsert of a batch (s->mu held, s no view, the arguments checked): one growth decision, then the batch kGroupBatch ids at a
// time, in order — a later occurrence of an id overrides an earlier one inside a launch (launch_group_upsert) and across launches.
void set_groups(pcv_searcher* s, const int64_t* ids, const int64_t* groups, int64_t n) {
    pcv_searcher::Groups& t = s->groups;
    if (n == 0) return;
    if (t.head.entries + n > kMaxGroupEntries)
        PCV_FAIL(PCV_ERR_UNSUPPORTED, "set_groups: %lld entries and %lld ids more exceed the table's limit of 2^30 entries",
                 (long long)t.head.entries, (long long)n);
    PCV_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    if (!t.d_head.p) {
        t.pin_head.ensure(1);
        t.d_head.ensure(1);
        *t.pin_head.p = t.head;
        PCV_HIP(hipMemcpyAsync(t.d_head.p, t.pin_head.p, sizeof(GroupHead), hipMemcpyHostToDevice, st));
    }
    hipEvent_t ev[2] = {nullptr, nullptr};  // (the call's own: a searcher without rows has none yet)
    const auto drop_events = at_exit([&] {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    });
    for (hipEvent_t& e : ev) PCV_HIP(hipEventCreate(&e));
    PCV_HIP(hipEventRecord(ev[0], st));
    uint64_t slots = std::max(t.slots, kMinGroupSlots);
    while (slots < 2 * (uint64_t)(t.head.entries + n)) slots *= 2;
    if (slots != t.slots) grow_groups(s, slots);
    auto trim = at_exit([&] { trim_group_scratch(s); });
    t.d_claim.ensure(t.slots);
    PCV_HIP(hipMemsetAsync(t.d_claim.p, 0, t.slots * sizeof(uint32_t), st));
    const size_t m_most = (size_t)std::min<int64_t>(n, kGroupBatch);
    t.d_batch.ensure(2 * m_most);
    t.d_slot.ensure(m_most);
    for (int64_t i0 = 0; i0 < n; i0 += kGroupBatch) {
        const size_t m = (size_t)std::min<int64_t>(kGroupBatch, n - i0);
        PCV_HIP(hipMemcpyAsync(t.d_batch.p, ids + i0, m * sizeof(int64_t), hipMemcpyHostToDevice, st));
        PCV_HIP(hipMemcpyAsync(t.d_batch.p + m_most, groups + i0, m * sizeof(int64_t), hipMemcpyHostToDevice, st));
        launch_group_upsert(st, t.keys, t.vals, (uint32_t)(t.slots - 1), t.d_claim.p, t.d_head.p, t.d_batch.p, t.d_batch.p + m_most,
                            (uint32_t)m, t.d_slot.p);
    }
    PCV_HIP(hipMemcpyAsync(t.pin_head.p, t.d_head.p, sizeof(GroupHead), hipMemcpyDeviceToHost, st));
    PCV_HIP(hipEventRecord(ev[1], st));
    PCV_HIP(hipStreamSynchronize(st));
    t.head = *t.pin_head.p;
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
    t.last_set_ms = ms;
}

// The searcher is as created: no table, every counter 0.
void clear_groups(pcv_searcher* s) {
    pcv_searcher::Groups& t = s->groups;
    PCV_HIP(hipSetDevice(s->ctx->device));
    PCV_HIP(hipStreamSynchronize(s->ctx->stream));
    if (t.keys) (void)hipFree(t.keys);
    if (t.vals) (void)hipFree(t.vals);
    t.keys = t.vals = nullptr;
    t.slots = 0;
    t.head = GroupHead{0, 0, -1, 0, 0};
    t.d_head.release();  // (the next set_groups uploads a fresh one)
    t.d_claim.release();
    t.rehashes = 0;
    t.last_set_ms = 0.0f;
}

// out[i] = group of ids[i] in the table of `owner` (locked by the caller); the scratch is owner's too.
void get_groups(pcv_searcher* owner, const int64_t* ids, int64_t n, int64_t* out) {
    pcv_searcher::Groups& t = owner->groups;
    if (!t.d_head.p) {  // nothing was ever set
        for (int64_t i = 0; i < n; ++i) out[i] = PCV_NO_GROUP;
        return;
    }
    PCV_HIP(hipSetDevice(owner->ctx->device));
    hipStream_t st = owner->ctx->stream;
    auto trim = at_exit([&] { trim_group_scratch(owner); });
    const size_t m_most = (size_t)std::min<int64_t>(n, kGroupBatch);
    t.d_batch.ensure(2 * m_most);
    for (int64_t i0 = 0; i0 < n; i0 += kGroupBatch) {
        const size_t m = (size_t)std::min<int64_t>(kGroupBatch, n - i0);
        PCV_HIP(hipMemcpyAsync(t.d_batch.p, ids + i0, m * sizeof(int64_t), hipMemcpyHostToDevice, st));
        launch_group_lookup(st, t.keys, t.vals, (uint32_t)(t.slots ? t.slots - 1 : 0), t.d_head.p, t.d_batch.p, (uint32_t)m, t.d_batch.p + m_most);
        PCV_HIP(hipMemcpyAsync(out + i0, t.d_batch.p + m_most, m * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PCV_HIP(hipStreamSynchronize(st));
    }
}

// search_distinct's walk (walk_ranked_lists) with membership as the relation: after each pass grouped_select_kernel looks the
// hits' ids up in the group table of `owner` (s itself, or the parent of a view; locked by the caller), keeps the first row of
// every group not kept yet and counts the others for the kept row of their group.  The state block is the one search_distinct
// uses, with the kept rows' group keys where that call has their norms — and these come down with the kept rows.
void search_grouped(pcv_searcher* s, const pcv_searcher* owner, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                    int k, int pool, int64_t* out_ids, float* out_scores, int64_t* out_groups, int32_t* out_counts, int32_t* out_collapsed,
                    int32_t* out_examined, uint8_t* out_more) {
    check_search_args(s, queries, n_queries, k, "search_grouped");
    s->stats = pcv_scan_stats{};  // (also when the kernel is refused)
    const SearchPlan plan = plan_search(s, source_ids, n_sources, n_queries);
    auto blank = [&](int q, int from) {
        for (int j = from; j < k; ++j) {
            if (out_ids) out_ids[(size_t)q * k + j] = -1;
            if (out_scores) out_scores[(size_t)q * k + j] = NAN;
            if (out_groups) out_groups[(size_t)q * k + j] = PCV_NO_GROUP;
            if (out_collapsed) out_collapsed[(size_t)q * k + j] = 0;
        }
    };
    if (!open_search(s, plan)) {
        for (int q = 0; q < n_queries; ++q) {
            blank(q, 0);
            if (out_counts) out_counts[q] = 0;
            if (out_examined) out_examined[q] = 0;
            if (out_more) out_more[q] = 0;
        }
        return;
    }
    using L = DistinctLayout;
    static_assert(sizeof(int64_t) == sizeof(double), "the group keys take the place of the norms");
    hipStream_t st = s->ctx->stream;
    s->d_distinct.ensure(L::total);
    s->pin_distinct.ensure(L::total);
    DistinctRec* rec = reinterpret_cast<DistinctRec*>(s->pin_distinct.p + L::off_rec);
    GroupedArgs args{};
    args.rec = reinterpret_cast<DistinctRec*>(s->d_distinct.p + L::off_rec);
    args.rec_host = rec;
    args.kept = reinterpret_cast<pcv_hit_dev*>(s->d_distinct.p + L::off_kept);
    args.collapsed = reinterpret_cast<int32_t*>(s->d_distinct.p + L::off_sim);
    args.kept_group = reinterpret_cast<int64_t*>(s->d_distinct.p + L::off_norm);
    args.keys = owner->groups.slots ? owner->groups.keys : nullptr;
    args.vals = owner->groups.vals;
    args.mask = owner->groups.slots ? (uint32_t)(owner->groups.slots - 1) : 0;
    args.side_val = owner->groups.head.side_val;
    args.num_results = k;
    const pcv_hit_dev* kept = reinterpret_cast<const pcv_hit_dev*>(s->pin_distinct.p + L::off_kept);
    const int32_t* collapsed = reinterpret_cast<const int32_t*>(s->pin_distinct.p + L::off_sim);
    const int64_t* kept_group = reinterpret_cast<const int64_t*>(s->pin_distinct.p + L::off_norm);
    for (int q0 = 0; q0 < n_queries; q0 += plan.qstep) {
        const int B = std::min(plan.qstep, n_queries - q0);
        const float* qs = queries + (size_t)q0 * s->D;
        const std::vector<uint8_t> more = walk_ranked_lists(s, plan, qs, B, pool, rec, args.rec, out_more != nullptr, [&] {
            launch_grouped_select(st, pass_params(s), reinterpret_cast<const ScanParams*>(s->d_pass.p), args);
        });
        PCV_HIP(hipMemcpyAsync(s->pin_distinct.p + L::off_kept, s->d_distinct.p + L::off_kept, L::total - L::off_kept, hipMemcpyDeviceToHost, st));
        PCV_HIP(hipStreamSynchronize(st));
        for (int q = 0; q < B; ++q) {
            const int n = (int)rec[q].kept;
            const size_t o = (size_t)(q0 + q) * k;
            for (int j = 0; j < n; ++j) {
                const pcv_hit_dev& h = kept[(size_t)q * kMaxK + j];
                if (out_ids) out_ids[o + j] = h.id;
                if (out_scores) out_scores[o + j] = reported_score(s->metric, s->D, h.score);
                if (out_groups) out_groups[o + j] = kept_group[(size_t)q * kMaxK + j];
                if (out_collapsed) out_collapsed[o + j] = collapsed[(size_t)q * kMaxK + j];
            }
            blank(q0 + q, n);
            if (out_counts) out_counts[q0 + q] = n;
            if (out_examined) out_examined[q0 + q] = (int32_t)rec[q].examined;
            if (out_more) out_more[q0 + q] = more[(size_t)q];
        }
    }
}

// The per-shard pass of the begin/end protocol; the caller holds s->mu.
void device_begin(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources, int k,
                  pcv_hit_dev* out, bool queries_on_device = false) {
    check_search_args(s, queries, n_queries, k, "search_device_begin");
    PCV_REQUIRE(!s->pending.active, "search_device_begin: the previous pass was not collected (search_device_end)");
    sync_view(s);
    const SearchPlan plan = plan_search(s, source_ids, n_sources, n_queries, true);
    // Only a condition every rank evaluates alike may refuse: the ranks of a sharded search must all
    // take the same protocol (the exchanged payload differs by the overflow record).
    if (n_queries > plan.qstep)
        PCV_FAIL(PCV_ERR_UNSUPPORTED, "search_device_begin: %d queries need more than one pass%s", n_queries,
                 s->wide_sharded ? " (wide sharded passes were allowed, but not every row of THIS rank has its int8 screening copy)" : "");
    const size_t n = (size_t)n_queries * k;
    if (!open_search(s, plan)) {  // (each rank builds mid copies by its own statistics: the copy changes no result and no protocol)
        // this shard holds none of the selected rows: hand over the same layout — empty lists and a clear
        // overflow record — from pinned memory; search_device_end waits for the copy like for a pass
        ensure_workspace(s);
        const pcv_hit_dev none{NAN, -1, -1};
        for (size_t i = 0; i < n; ++i) s->pin->hits[i] = none;
        s->pin->hits[n] = pcv_hit_dev{0.0, 0, 0};
        PCV_HIP(hipMemcpyAsync(out, s->pin->hits, (n + 1) * sizeof(pcv_hit_dev), hipMemcpyHostToDevice, s->ctx->stream));
        s->pending.active = true;
        s->pending.done = true;
        return;
    }
    PassRequest pass = PassRequest(queries, n_queries, plan.segs, plan.kernel).top_k(k, out, false, out + n);
    if (queries_on_device) pass.where = PassRequest::kDevice;
    enqueue_pass(s, pass);
    if (s->view_parent) launch_view_remap(s->ctx->stream, out, (int64_t)n, s->d_ppos.p, s->view_rows);  // (before any exchange)
}

// ---- views (pcv_searcher_create_view; DESIGN.md §3 "Views") ----
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

// A graph captured over rows that are about to move or to be freed must not replay: the next passes capture afresh.
void drop_pass_graph(pcv_searcher* s) {
    if (s->graph_exec) (void)hipGraphExecDestroy(s->graph_exec);
    s->graph_exec = nullptr;
    s->graph_shape = s->last_shape = pcv_searcher::PassShape{};
    s->shape_seen = 0;
}

// the screening copy a view keeps: the kind its parent holds for all of its rows, none if the parent holds none
int view_screen_mode(const pcv_searcher* p) {
    return p->copies_kind == 2 ? PCV_SCREEN_COPY_INT8 : (p->copies_kind == 1 ? PCV_SCREEN_COPY_BF16 : PCV_SCREEN_COPY_OFF);
}

void drop_view_rows(pcv_searcher* v) {
    for (auto& src : v->sources)
        for (auto& g : src.segs) free_segment(g);
    v->sources.clear();
    v->d_ppos.release();
    v->view_rows = 0;
    v->copies_kind = 0;
    v->mids_present = false;
}

// A view segment of exactly `rows` rows (rounded up to whole blocks); every byte of it is written by view_gather_kernel.
Segment alloc_view_segment(pcv_searcher* v, int64_t rows) {
    PCV_REQUIRE(rows > 0 && rows <= kMaxSegRows, "view: a source of %lld rows is out of range", (long long)rows);
    Segment g;
    const uint32_t nblk = (uint32_t)((rows + kBlockRows - 1) / kBlockRows);
    g.cap_rows = nblk * kBlockRows;
    try {
        PCV_HIP(hipMalloc((void**)&g.blk, (size_t)nblk * v->D4 * 32 * sizeof(float4)));
        PCV_HIP(hipMalloc((void**)&g.scale, (size_t)g.cap_rows * sizeof(float)));
        PCV_HIP(hipMalloc((void**)&g.ids, (size_t)g.cap_rows * sizeof(int64_t)));
    } catch (...) {
        free_segment(g);
        throw;
    }
    g.nrows = g.scaled_rows = (uint32_t)rows;
    return g;
}

// (Re)build view v from its parent p (p->mu held): per parent source, the rows whose id is in the allow list become ONE view
// segment, in parent source order and row order — so a view position grows with the parent position it stands for —, copied
// with their scales (a hidden or unsearchable row keeps scale 0).  Then the screening copies the parent holds, and a mid copy if
// the parent's mode is ON, are made from the view's own blocks: an int8 block scale depends on which rows share the block.  All
// or nothing: if anything fails the view holds no rows (and stays stale, so its next call tries again).
void build_view(pcv_searcher* v, pcv_searcher* p) {
    PCV_REQUIRE(!p->dirty, "view: its parent has rows added or cleared without pcv_searcher_finalize");
    hipStream_t st = v->ctx->stream;
    PCV_HIP(hipSetDevice(v->ctx->device));
    PCV_HIP(hipStreamSynchronize(st));  // (a pass of the view may still read the old rows)
    drop_view_rows(v);
    drop_pass_graph(v);
    v->screen_copy = view_screen_mode(p);
    v->screen_copy_gave_way = false;
    v->mid_copy = p->mid_copy == PCV_MID_COPY_ON ? PCV_MID_COPY_ON : PCV_MID_COPY_OFF;
    v->max_norm = p->max_norm;  // bounds every row of the parent, so every row of the view
    for (auto& e : v->ev)
        if (!e) PCV_HIP(hipEventCreate(&e));
    PCV_HIP(hipEventRecord(v->ev[0], st));
    struct Part {
        const Segment* g;
        DevBuf<uint32_t> sel;  // the rows of g, ascending
        uint32_t n;
    };
    struct SrcPlan {
        int64_t id;
        std::vector<Part> parts;
        int64_t rows;
    };
    std::vector<SrcPlan> plan;  // (this and the scratch below are freed by scope, behind the catch's synchronise)
    DevBuf<uint32_t> flags4, tiles, total;
    IdBatch b;
    b.ids = &v->view_ids;
    const auto give_back = at_exit([v] { v->d_idtab.release(); });
    int64_t rows = 0;
    try {
        // 1. which rows: an id column is matched on the device (order-keeping selection), implicit ids (id0 + row) on the host
        for (const auto& src : p->sources) {
            SrcPlan sp{src.id, {}, 0};
            for (const auto& g : src.segs) {
                if (g.nrows == 0 || v->view_ids.empty()) continue;
                Part pt{&g, {}, 0};
                if (!g.ids) {
                    const auto in = implicit_range(v->view_ids, g, 0, g.nrows);
                    std::vector<uint32_t> sel;
                    for (size_t i = in.first; i < in.second; ++i) sel.push_back((uint32_t)(v->view_ids[i] - g.id0));
                    pt.n = (uint32_t)sel.size();
                    if (pt.n) {
                        pt.sel.ensure(pt.n);
                        PCV_HIP(hipMemcpyAsync(pt.sel.p, sel.data(), sel.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
                        PCV_HIP(hipStreamSynchronize(st));  // (sel goes out of scope)
                    }
                } else {
                    upload_id_batch(v, b);
                    const uint32_t nt = view_tiles(g.nrows);
                    flags4.ensure((size_t)nt * 256);
                    tiles.ensure(nt);
                    total.ensure(1);
                    launch_view_select(st, g.ids, g.nrows, v->d_idtab.p, b.tmask, b.has_empty, flags4.p, tiles.p, total.p);
                    PCV_HIP(hipMemcpyAsync(&pt.n, total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                    PCV_HIP(hipStreamSynchronize(st));
                    if (pt.n) {
                        pt.sel.ensure(pt.n);
                        launch_view_compact(st, flags4.p, tiles.p, g.nrows, pt.sel.p);
                        PCV_HIP(hipStreamSynchronize(st));  // (flags4 / tiles are the next segment's)
                    }
                }
                if (pt.n) {
                    sp.rows += pt.n;
                    sp.parts.push_back(std::move(pt));
                }
            }
            if (sp.rows) plan.push_back(std::move(sp));
        }
        // 2. every buffer: the view's segments and the parent positions of their rows
        for (const auto& sp : plan) {
            Segment g = alloc_view_segment(v, sp.rows);
            v->sources.emplace_back();
            v->sources.back().id = sp.id;
            v->sources.back().segs.push_back(g);
            rows += sp.rows;
        }
        if (rows) v->d_ppos.ensure((size_t)rows);
        assign_positions(v);  // (shard offset 0: a view numbers its rows from 0)
        // 3. the rows, then the padding of each segment's last block
        for (size_t i = 0; i < plan.size(); ++i) {
            Segment& dst = v->sources[i].segs[0];
            int64_t* ppos = v->d_ppos.p + dst.pos0;
            uint32_t at = 0;
            for (const Part& pt : plan[i].parts) {
                launch_view_gather(st, pt.g->blk, pt.g->scale, pt.g->ids, pt.g->id0, pt.g->pos0, pt.sel.p, pt.n, v->D4, at, at + pt.n, dst.blk,
                                   dst.scale, dst.ids, ppos);
                at += pt.n;
            }
            launch_view_gather(st, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, v->D4, at, dst.cap_rows, dst.blk, dst.scale, dst.ids, ppos);
        }
        // 4. the copies, from the view's own blocks, as a finalize of these rows makes them
        for (auto& src : v->sources) build_screening_copies(v, src);
        build_six_copies(v);
        if (v->mid_copy == PCV_MID_COPY_ON && rows) build_mid_copies(v, true);
        refresh_copy_state(v);
        PCV_HIP(hipEventRecord(v->ev[3], st));
        PCV_HIP(hipStreamSynchronize(st));
        PCV_HIP(hipGetLastError());
    } catch (...) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(st);
        drop_view_rows(v);
        throw;
    }
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, v->ev[0], v->ev[3]);
    v->view_build_ms = ms;
    v->view_rows = rows;
    v->view_gen = p->gen;
}

}  // namespace

// Every call on a view starts here (v->mu held): if its parent changed since the rows were copied, they are copied again, under
// the parent's lock.
void pcv::sync_view(pcv_searcher* v) {
    if (!v->view_parent) return;
    pcv_searcher* p = v->view_parent;
    std::lock_guard<std::mutex> lk(p->mu);
    if (v->view_gen == p->gen) return;
    build_view(v, p);
    v->view_refreshes += 1;
}

namespace {

// ---- search by example (pcv_searcher_like_queries / _search_like; DESIGN.md §3 "Search by example") ----
// What both entry points check before anything touches the searcher or the device; returns the number of examples.
int64_t check_like_args(const pcv_searcher* s, const int64_t* example_ids, const float* weights, const int64_t* offsets, int n_queries,
                        const char* who) {
    PCV_REQUIRE(s != nullptr, "%s: searcher is NULL", who);
    PCV_REQUIRE(n_queries >= 0, "%s: n_queries < 0", who);
    PCV_REQUIRE(offsets != nullptr, "%s: offsets is NULL", who);
    PCV_REQUIRE(offsets[0] == 0, "%s: offsets[0] must be 0", who);
    for (int q = 0; q < n_queries; ++q)
        PCV_REQUIRE(offsets[q + 1] >= offsets[q], "%s: offsets are not ascending (offsets[%d] < offsets[%d])", who, q + 1, q);
    const int64_t n = offsets[n_queries];
    PCV_REQUIRE(n <= 0x7fffffff, "%s: %lld examples in one call", who, (long long)n);
    PCV_REQUIRE(example_ids != nullptr || n == 0, "%s: example ids NULL with %lld examples", who, (long long)n);
    if (weights)
        for (int64_t i = 0; i < n; ++i) PCV_REQUIRE(std::isfinite(weights[i]), "%s: weight %lld is not finite", who, (long long)i);
    return n;
}

// The searcher the examples are looked up in (a view: its parent — an example need not be among the allowed items), locked, in
// the state both calls need.  The caller holds s->mu and has brought a view up to date.
std::unique_lock<std::mutex> lock_like_owner(pcv_searcher* s, pcv_searcher*& owner, const char* who) {
    PCV_REQUIRE(!s->pending.active, "%s: a queued pass has not been collected", who);
    owner = s->view_parent ? s->view_parent : s;
    std::unique_lock<std::mutex> lk;
    if (owner != s) lk = std::unique_lock<std::mutex>(owner->mu);
    PCV_REQUIRE(!owner->dirty, "%s: pending rows; call pcv_searcher_finalize first", who);
    PCV_REQUIRE(!owner->pending.active, "%s: a queued pass has not been collected", who);
    return lk;
}

// What the lookup of a call's examples gives back to the host.
struct LikeBuilt {
    std::vector<float> vectors;         // [n_queries][D], if asked for
    std::vector<int64_t> member_rows;   // [n_queries] rows that went into each query
    std::vector<int64_t> carrier_rows;  // [n_queries] ... plus the rows staged under PCV_STAGING_SOURCE that carry one of its ids
    std::vector<uint8_t> found;         // [examples]
};

// Query vectors from stored items (p->mu held, p no view): the distinct ids of the call are looked up once in every segment
// (find_slots: an id column is streamed against the batch's table, implicit ids are arithmetic), each id's rows listed in
// ascending global position, the lists expanded per query in the order the examples were given, and like_queries_kernel sums
// the rows.  Reads rows and ids only.
void build_like_queries(pcv_searcher* p, const int64_t* example_ids, const float* weights, const int64_t* offsets, int n_queries,
                        bool want_host, void* d_out, LikeBuilt& out) {
    const int64_t n = offsets[n_queries];
    out.member_rows.assign((size_t)n_queries, 0);
    out.carrier_rows.assign((size_t)n_queries, 0);
    out.found.assign((size_t)n, 0);
    if (want_host) out.vectors.assign((size_t)n_queries * p->D, 0.0f);
    if (n_queries == 0) return;
    PCV_HIP(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->stream;
    // 1. one slot per distinct id
    std::vector<int64_t> uniq(example_ids, example_ids + n);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    std::vector<uint32_t> slot_of(uniq.size());
    std::iota(slot_of.begin(), slot_of.end(), 0u);
    // 2. the rows of every slot: (segment of the table, row), ascending in global position — sources and segments are walked in
    //    the order assign_positions numbers them, rows ascending inside a segment
    std::vector<SegDesc> segs;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> rows_of(uniq.size());
    std::vector<int64_t> staged_of(uniq.size(), 0);
    if (!uniq.empty()) {
        IdBatch b;
        b.ids = &uniq;
        b.slots = &slot_of;
        for (const auto& src : p->sources)
            for (const auto& g : src.segs) {
                if (g.nrows == 0) continue;
                auto pr = find_slots(p, g, b);
                if (pr.empty()) continue;
                if (src.id == PCV_STAGING_SOURCE) {  // nobody's rows yet: no members, but a search that names the source may meet them
                    for (const auto& x : pr) staged_of[x.first] += 1;
                    continue;
                }
                std::sort(pr.begin(), pr.end(), [](const auto& a, const auto& c) { return a.second < c.second; });
                PCV_REQUIRE(segs.size() < 0x7fffffffu, "like_queries: too many segments");
                const uint32_t si = (uint32_t)segs.size();
                SegDesc d{};  // (like_queries_kernel reads the rows and their number; no copy is involved)
                d.blk = g.blk;
                d.scale = g.scale;
                d.ids = g.ids;
                d.id0 = g.id0;
                d.pos0 = g.pos0;
                d.nrows = g.nrows;
                d.nblocks = g.nblocks();
                segs.push_back(d);
                for (const auto& x : pr) rows_of[x.first].push_back({si, x.second});
            }
    }
    // 3. the member list, per query in the order given
    std::vector<LikeMember> members;
    std::vector<uint32_t> first((size_t)n_queries + 1, 0);
    for (int q = 0; q < n_queries; ++q) {
        for (int64_t i = offsets[q]; i < offsets[q + 1]; ++i) {
            const size_t slot = (size_t)(std::lower_bound(uniq.begin(), uniq.end(), example_ids[i]) - uniq.begin());
            const auto& rows = rows_of[slot];
            out.found[(size_t)i] = rows.empty() ? 0 : 1;
            out.carrier_rows[(size_t)q] += (int64_t)rows.size() + staged_of[slot];
            PCV_REQUIRE(members.size() + rows.size() <= 0x7fffffffu, "like_queries: more than 2^31 member rows in one call");
            for (const auto& r : rows) members.push_back(LikeMember{r.first, r.second, weights ? weights[i] : 1.0f});
        }
        first[(size_t)q + 1] = (uint32_t)members.size();
        out.member_rows[(size_t)q] = (int64_t)(first[(size_t)q + 1] - first[(size_t)q]);
    }
    // 4. the sums
    DevBuf<SegDesc> d_segs;
    DevBuf<LikeMember> d_members;
    DevBuf<uint32_t> d_first;
    DevBuf<float> d_vec;
    try {
        d_segs.ensure(segs.size() + 1);
        d_members.ensure(members.size() + 1);
        d_first.ensure(first.size());
        d_vec.ensure((size_t)n_queries * p->D);
        if (!segs.empty()) PCV_HIP(hipMemcpyAsync(d_segs.p, segs.data(), segs.size() * sizeof(SegDesc), hipMemcpyHostToDevice, st));
        if (!members.empty())
            PCV_HIP(hipMemcpyAsync(d_members.p, members.data(), members.size() * sizeof(LikeMember), hipMemcpyHostToDevice, st));
        PCV_HIP(hipMemcpyAsync(d_first.p, first.data(), first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        launch_like_queries(st, d_segs.p, (int)segs.size(), d_members.p, d_first.p, n_queries, p->D, p->D4, d_vec.p);
        const size_t bytes = (size_t)n_queries * p->D * sizeof(float);
        if (want_host) PCV_HIP(hipMemcpyAsync(out.vectors.data(), d_vec.p, bytes, hipMemcpyDeviceToHost, st));
        if (d_out) PCV_HIP(hipMemcpyAsync(d_out, d_vec.p, bytes, hipMemcpyDeviceToDevice, st));
        PCV_HIP(hipStreamSynchronize(st));
        PCV_HIP(hipGetLastError());
    } catch (...) {
        (void)hipStreamSynchronize(st);  // (before the buffers queued work may still read are freed)
        throw;
    }
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
    if (s->groups.keys) (void)hipFree(s->groups.keys);
    if (s->groups.vals) (void)hipFree(s->groups.vals);
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
        PCV_REQUIRE(!parent->dirty, "create_view: pending rows; call pcv_searcher_finalize first");
        PCV_REQUIRE(!parent->pending.active, "create_view: a queued pass has not been collected");
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
        v->view_ids.swap(allow);
        v->view_parent = parent;
        parent->live_views.fetch_add(1);  // (given back by destroy_searcher, also if the build fails)
        try {
            build_view(v, parent);
        } catch (...) {
            destroy_searcher(v);
            throw;
        }
        *out_view = v;
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
        if (out_ids) *out_ids = (int64_t)v->view_ids.size();
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
        PCV_REQUIRE(s != nullptr, "search_distinct: searcher is NULL");
        PCV_REQUIRE(queries != nullptr && n_queries > 0, "search_distinct: no queries");
        PCV_REQUIRE(num_results >= 1 && num_results <= (int)PCV_MAX_RESULTS, "search_distinct: num_results %d outside [1,%d]", num_results,
                    (int)PCV_MAX_RESULTS);
        PCV_REQUIRE(pool >= num_results && pool <= (int)PCV_MAX_DISTINCT_POOL, "search_distinct: pool %d outside [num_results = %d, %d]", pool,
                    num_results, (int)PCV_MAX_DISTINCT_POOL);
        PCV_REQUIRE(threshold == threshold, "search_distinct: threshold is NaN");
        PCV_REQUIRE(threshold > -1.0f && threshold <= 1.0f, "search_distinct: threshold %g outside (-1, 1]", (double)threshold);
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "search_distinct: a pass queued by search_device_begin has not been collected");
        sync_view(s);
        search_distinct(s, queries, n_queries, source_ids, n_sources, num_results, threshold, pool, out_ids, out_scores, out_counts, out_similar,
                        out_examined, out_more);
    });
}

pcv_status pcv_searcher_search_diverse(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                       int num_results, float lambda, int pool, int64_t* out_ids, float* out_scores, double* out_marginal,
                                       int32_t* out_ranks, int32_t* out_counts, int32_t* out_examined, uint8_t* out_exact) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "search_diverse: searcher is NULL");
        PCV_REQUIRE(queries != nullptr && n_queries > 0, "search_diverse: no queries");
        PCV_REQUIRE(num_results >= 1 && num_results <= (int)PCV_MAX_RESULTS, "search_diverse: num_results %d outside [1,%d]", num_results,
                    (int)PCV_MAX_RESULTS);
        PCV_REQUIRE(pool >= num_results && pool <= (int)PCV_MAX_DIVERSE_POOL, "search_diverse: pool %d outside [num_results = %d, %d]", pool,
                    num_results, (int)PCV_MAX_DIVERSE_POOL);
        PCV_REQUIRE(lambda == lambda, "search_diverse: lambda is NaN");
        PCV_REQUIRE(lambda >= 0.0f && lambda <= 1.0f, "search_diverse: lambda %g outside [0, 1]", (double)lambda);
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "search_diverse: a pass queued by search_device_begin has not been collected");
        sync_view(s);
        search_diverse(s, queries, n_queries, source_ids, n_sources, num_results, lambda, pool, out_ids, out_scores, out_marginal, out_ranks,
                       out_counts, out_examined, out_exact);
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
        set_groups(s, ids, groups, n);
    });
}

pcv_status pcv_searcher_clear_groups(pcv_searcher* s) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "clear_groups: searcher is NULL");
        refuse_view(s, "clear_groups");
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "clear_groups: a queued pass has not been collected");
        clear_groups(s);
    });
}

pcv_status pcv_searcher_get_groups(pcv_searcher* s, const int64_t* ids, int64_t n, int64_t* out_groups) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "get_groups: searcher is NULL");
        PCV_REQUIRE(n >= 0 && ((ids != nullptr && out_groups != nullptr) || n == 0), "get_groups: bad lists (NULL with n > 0, or n < 0)");
        pcv_searcher* owner = s->view_parent ? s->view_parent : s;
        std::lock_guard<std::mutex> lk(owner->mu);
        PCV_REQUIRE(!owner->pending.active, "get_groups: a queued pass has not been collected");
        get_groups(owner, ids, n, out_groups);
    });
}

pcv_status pcv_searcher_group_stats(pcv_searcher* s, pcv_group_stats* out) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr && out != nullptr, "group_stats: NULL argument");
        pcv_searcher* owner = s->view_parent ? s->view_parent : s;
        std::lock_guard<std::mutex> lk(owner->mu);
        const pcv_searcher::Groups& t = owner->groups;
        *out = pcv_group_stats{t.head.ids, t.head.entries, (int64_t)t.slots, t.rehashes, t.last_set_ms};
    });
}

pcv_status pcv_searcher_search_grouped(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                       int num_results, int pool, int64_t* out_ids, float* out_scores, int64_t* out_groups,
                                       int32_t* out_counts, int32_t* out_collapsed, int32_t* out_examined, uint8_t* out_more) {
    return guarded([&] {
        PCV_REQUIRE(s != nullptr, "search_grouped: searcher is NULL");
        PCV_REQUIRE(queries != nullptr && n_queries > 0, "search_grouped: no queries");
        PCV_REQUIRE(num_results >= 1 && num_results <= (int)PCV_MAX_RESULTS, "search_grouped: num_results %d outside [1,%d]", num_results,
                    (int)PCV_MAX_RESULTS);
        PCV_REQUIRE(pool >= num_results && pool <= (int)PCV_MAX_GROUPED_POOL, "search_grouped: pool %d outside [num_results = %d, %d]", pool,
                    num_results, (int)PCV_MAX_GROUPED_POOL);
        std::lock_guard<std::mutex> lk(s->mu);
        PCV_REQUIRE(!s->pending.active, "search_grouped: a pass queued by search_device_begin has not been collected");
        sync_view(s);
        // (a view reads its parent's table: the parent stays locked while the kernels may follow its pointers)
        std::unique_lock<std::mutex> plk;
        if (s->view_parent) plk = std::unique_lock<std::mutex>(s->view_parent->mu);
        search_grouped(s, s->view_parent ? s->view_parent : s, queries, n_queries, source_ids, n_sources, num_results, pool, out_ids,
                       out_scores, out_groups, out_counts, out_collapsed, out_examined, out_more);
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
        check_search_args(s, queries, n_queries, k, "search_sharded");
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
