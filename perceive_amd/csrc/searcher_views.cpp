// searcher_views.cpp — views (pcv_searcher_create_view; DESIGN.md §3 "Views"): the copy of the allowed rows of a parent and
// its refresh.  build_view is called with the parent's lock held, sync_view with the view's own (it takes the parent's).
#include "searcher_calls.h"

namespace pcv {
namespace {

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

}  // namespace

// (Re)build view v from its parent p (p->mu held): per parent source, the rows whose id is in the allow list (a predicate view:
// whose id's value passes the predicate) become ONE view
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
        // 1. which rows.  An id-list view: an id column is matched on the device (order-keeping selection), implicit ids (id0 + row)
        // on the host.  A predicate view: every segment alike on the device — where_mark_kernel tests the value of each row's id
        // against the predicate (the parent's value table; p->mu is held), the scan and the compaction follow as for an id column.
        const ValueTable vt = value_table_of(p);
        for (const auto& src : p->sources) {
            SrcPlan sp{src.id, {}, 0};
            for (const auto& g : src.segs) {
                if (g.nrows == 0 || (!v->view_by_value && v->view_ids.empty())) continue;
                Part pt{&g, {}, 0};
                if (v->view_by_value) {
                    const uint32_t nt = view_tiles(g.nrows);
                    flags4.ensure((size_t)nt * 256);
                    tiles.ensure((size_t)nt * 2);
                    total.ensure(1);
                    launch_where_mark(st, g.ids, g.id0, g.scale, g.nrows, vt, v->view_where, flags4.p, tiles.p, tiles.p + nt);
                    launch_view_scan(st, tiles.p, nt, total.p);
                    PCV_HIP(hipMemcpyAsync(&pt.n, total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                    PCV_HIP(hipStreamSynchronize(st));
                    if (pt.n) {
                        pt.sel.ensure(pt.n);
                        launch_view_compact(st, flags4.p, tiles.p, g.nrows, pt.sel.p);
                        PCV_HIP(hipStreamSynchronize(st));  // (flags4 / tiles are the next segment's)
                    }
                } else if (!g.ids) {
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
    v->view_values_gen = p->values_gen;
}

// Every call on a view starts here (v->mu held): if its parent changed since the rows were copied, they are copied again, under
// the parent's lock.
void sync_view(pcv_searcher* v) {
    if (!v->view_parent) return;
    pcv_searcher* p = v->view_parent;
    std::lock_guard<std::mutex> lk(p->mu);
    // (an id-list view never looks at the value table: set_values leaves it as it is)
    if (v->view_gen == p->gen && (!v->view_by_value || v->view_values_gen == p->values_gen)) return;
    build_view(v, p);
    v->view_refreshes += 1;
}

}  // namespace pcv
