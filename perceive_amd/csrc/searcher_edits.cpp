// searcher_edits.cpp — changes to stored rows by item id: looking a batch of ids up in the segments (IdBatch, searcher_internal.h),
// and hide, unhide, update and remove.  Called by the entry points of searcher.cpp, finalize, the view build and search by
// example, always with s->mu held and no pass in flight.
#include <cstdlib>
#include <cstring>
#include <iterator>

#include "searcher_internal.h"

namespace pcv {

// ---- hidden items (pcv_searcher_hide_ids; DESIGN.md §3 "Hidden items") ----
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
static uint32_t match_id_column(pcv_searcher* s, const Segment& g, uint32_t r0, uint32_t r1, IdBatch& b, std::vector<uint32_t>* rows = nullptr,
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
static uint32_t find_rows(pcv_searcher* s, const Segment& g, uint32_t r0, uint32_t r1, IdBatch& b) {
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

static void hide_found(pcv_searcher* s, Segment& g, uint32_t n) {
    launch_hide_rows(s->ctx->stream, s->d_hrows.p, n, g.scale, g.blk8, g.blk16, g.copied_rows, g.mid16 ? g.scale16 : nullptr, g.mid_rows,
                     s->D4);
}

// The rows of [r0, r1) of g whose id is in the batch are hidden; how many -> (finalize: the new rows of a searcher with hidden
// ids).  The stream has drained on return: s->d_hrows is the next lookup's.
uint32_t hide_rows_in(pcv_searcher* s, Segment& g, uint32_t r0, uint32_t r1, IdBatch& b) {
    const uint32_t n = find_rows(s, g, r0, r1, b);
    if (n) hide_found(s, g, n);
    PCV_HIP(hipStreamSynchronize(s->ctx->stream));
    return n;
}

// The rows come back: their scales, then the copies (repair_copies).
static void unhide_found(pcv_searcher* s, Segment& g, uint32_t n) {
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
namespace {
struct UpdateSeg {
    Segment* g = nullptr;
    std::vector<uint32_t> rows, slots, blocks;
    size_t off = 0, boff = 0;
};
}  // namespace

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
    read_max_norm(s);
    return (int64_t)total;
}

// ---- removed items (pcv_searcher_remove_ids; DESIGN.md §3 "Removed items") ----
// One segment that loses rows: the flags of its rows (1 = the row stays, view_mark_kernel's layout) and the tiles' offsets on the
// device, the offsets on the host as well (off[t] = rows that stay in front of tile t; off[tiles] = keep).
namespace {
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
}  // namespace

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

}  // namespace pcv
