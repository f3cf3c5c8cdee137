// reach_kernels.hip — the device steps of pcv_searcher_reach_tree (DESIGN.md §4 "Reach tree") that the linkage tree does not have:
// the spanning tree of the participating rows under the mutual-reachability weight w(a, b) = min(core(a), core(b), c(a, b)), exact, in
// the Borůvka rounds of linkage_kernels.hip with the cap applied.  The norms come from selfjoin_prep_kernel, the candidates of the
// core step from the neighbours' bound, threshold, list and rescore (neighbors_kernels.hip) with k = j; begin, cert, threshold, choose,
// merge, flatten and settle are the linkage kernels themselves (launch_linkage_*), which see the LinkageArgs inside ReachArgs, and so
// is the screen: reach_screen_kernel<NT, LIST> of linkage_kernels.hip, which launch_linkage_bound and launch_linkage_list run when they are given
// klo / khi.  Its bound pass raises min(s, klo[a], klo[b]) instead of s; in its list pass (owner a, partner b) is a candidate iff
// both take part, s >= thr[comp[a]] (or a row is wild), comp[a] != comp[b], khi[a] >= thr and khi[b] >= thr.  Here:
//
//   reach_core_kernel                   a wave per launch row: the j-th largest f64 image among the row's rescored candidates, found
//                                       bit by bit from the top -> core[launch row]
//   reach_images_kernel                 klo = core rounded down to f32, khi = core rounded up (both +inf for j == 0, -inf for a row
//                                       that takes no part, whose core is NaN)
//   reach_rescore_kernel                c as linkage_rescore_kernel computes it, w = min(core[a], core[b], c) in f64, the 64-bit
//                                       atomic max of f64_key(w); launch_linkage_choose then takes the lowest pair that reaches it
//   reach_rows_kernel, _edges           the outputs by position; an edge's c is computed once more
#include "device_access.h"
#include "launch_rows.h"
#include "row_jobs.h"

namespace pcv {
namespace {

// a wave per launch row.  The row's stretch of sorted_key holds the image of c with every partner the neighbours' list pass left it:
// all of its j best are among them.  The largest T with at least j images >= T is the j-th largest image, ties counted as often as
// they occur.  A participating row with fewer than j images is counted in *short_rows (for the host, an internal error).
__global__ __launch_bounds__(256) void reach_core_kernel(const ReachArgs a, uint32_t launch_rows) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= launch_rows) return;  // (the whole wave)
    const int lane = threadIdx.x & 63;
    if (gld(&a.l.rinv[row]) == 0.0f) {
        if (lane == 0) gst(&a.core[row], (double)__builtin_nanf(""));
        return;
    }
    const uint32_t e0 = gld(&a.row_off[row]), e1 = gld(&a.row_off[row + 1]);
    unsigned long long T = 0;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long cand = T | (1ull << bit);
        int n = 0;
        for (uint32_t e = e0; e < e1; e += 64) {  // (wave-uniform bounds: the whole wave votes)
            const uint32_t i = e + (uint32_t)lane;
            const unsigned long long key = i < e1 ? gld(&a.sorted_key[i]) : 0ull;
            n += __builtin_popcountll(__ballot(key >= cand));
        }
        if (n >= a.k) T = cand;
    }
    if (lane != 0) return;
    if (T == 0) {
        (void)g_atomic_add64(a.short_rows, 1ull);
        gst(&a.core[row], (double)__builtin_nanf(""));
    } else {
        gst(&a.core[row], key_f64(T));
    }
}

// one thread per launch row.  have_core == 0 (j == 0): core = +inf for the rows that take part, NaN for the others
__global__ __launch_bounds__(256) void reach_images_kernel(const ReachArgs a, uint32_t launch_rows, int have_core) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= launch_rows) return;
    const bool part = gld(&a.l.rinv[i]) != 0.0f;
    double core;
    if (have_core) {
        core = gld(&a.core[i]);
    } else {
        core = part ? (double)__builtin_inff() : (double)__builtin_nanf("");
        gst(&a.core[i], core);
    }
    const bool ok = part && core == core;
    gst(&a.klo[i], ok ? __double2float_rd(core) : -__builtin_inff());
    gst(&a.khi[i], ok ? __double2float_ru(core) : -__builtin_inff());
}

// one thread per candidate: the canonical cosine (linkage_rescore_kernel's arithmetic), capped by the two cores; the image of w is
// kept for the choose step and raised into the owner's component
__global__ __launch_bounds__(256) void reach_rescore_kernel(const ScanParams* __restrict__ pp, const ReachArgs ra_) {
    const ScanParams& p = *pp;
    const LinkageArgs& a = ra_.l;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_cand) return;
    const uint64_t cd = gld(&a.cand[i]);
    const uint32_t la = (uint32_t)(cd >> 32), lb = (uint32_t)cd;
    const RowRef ra = row_ref(p, la), rb = row_ref(p, lb);
    const float4* y[1] = {rb.x};
    double acc[1];
    pair_sums<1>(ra.x, y, p.D4, acc, 32);
    const double cc = finish_score(PCV_METRIC_COSINE, acc[0], gld(&a.norm[la]), gld(&a.norm[lb]));
    const double ka = gld(&ra_.core[la]), kb = gld(&ra_.core[lb]);
    double w = cc;
    w = ka < w ? ka : w;
    w = kb < w ? kb : w;
    const unsigned long long key = (cc == cc && ka == ka && kb == kb) ? f64_key(w) : 0ull;  // (both rows take part: all three are numbers)
    gst(&a.cand_key[i], key);
    if (key) g_atomic_max64(&a.best_key[gld(&a.comp[la])], key);
}

__global__ __launch_bounds__(256) void reach_rows_kernel(const ScanParams* __restrict__ pp, const ReachArgs ra_) {
    const ScanParams& p = *pp;
    const LinkageArgs& a = ra_.l;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)p.total_blocks * 32) return;
    const RowRef r = row_ref(p, (uint32_t)i);
    if (r.row >= gld(&r.sg->nrows)) return;
    const int64_t o = gld(&a.seg_out0[r.sg - p.seg]) + (int64_t)r.row;
    gst(&a.out_ids[o], row_id(r));
    gst(&a.out_part[o], (int8_t)(gld(&a.rinv[i]) != 0.0f ? 1 : 0));
    gst(&ra_.out_core[o], gld(&ra_.core[i]));
}

__global__ __launch_bounds__(256) void reach_edges_kernel(const ScanParams* __restrict__ pp, const ReachArgs ra_) {
    const ScanParams& p = *pp;
    const LinkageArgs& a = ra_.l;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_edges) return;
    const unsigned long long pair = gld(&a.edge_pair[i]);
    const uint32_t la = (uint32_t)(pair >> 32), lb = (uint32_t)pair;
    const RowRef ra = row_ref(p, la), rb = row_ref(p, lb);
    const float4* y[1] = {rb.x};
    double acc[1];
    pair_sums<1>(ra.x, y, p.D4, acc, 32);
    PCV_GLOBAL ReachEdge* out = (PCV_GLOBAL ReachEdge*)&ra_.out_edges[i];
    out->w = key_f64(gld(&a.edge_key[i]));
    out->c = finish_score(PCV_METRIC_COSINE, acc[0], gld(&a.norm[la]), gld(&a.norm[lb]));
    out->pos_a = gld(&a.seg_out0[ra.sg - p.seg]) + (int64_t)ra.row;
    out->pos_b = gld(&a.seg_out0[rb.sg - p.seg]) + (int64_t)rb.row;
    out->id_a = row_id(ra);
    out->id_b = row_id(rb);
}

}  // namespace

void launch_reach_core(hipStream_t st, const ScanParams& p, const ReachArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t launch_rows = p.total_blocks * 32;
    if (a.k >= 1) reach_core_kernel<<<cdiv64((int64_t)launch_rows, 4), 256, 0, st>>>(a, launch_rows);
    reach_images_kernel<<<cdiv64((int64_t)launch_rows, 256), 256, 0, st>>>(a, launch_rows, a.k >= 1 ? 1 : 0);
    PCV_LAUNCHED();
}

void launch_reach_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const ReachArgs& a) {
    if (a.l.n_cand == 0) return;
    reach_rescore_kernel<<<cdiv64((int64_t)a.l.n_cand, 256), 256, 0, st>>>(dp, a);
    launch_linkage_choose(st, a.l);
}

void launch_reach_output(hipStream_t st, const ScanParams& p, const ScanParams* dp, const ReachArgs& a) {
    if (p.total_blocks == 0) return;
    reach_rows_kernel<<<cdiv64((int64_t)p.total_blocks * 32, 256), 256, 0, st>>>(dp, a);
    if (a.l.n_edges) reach_edges_kernel<<<cdiv64((int64_t)a.l.n_edges, 256), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

}  // namespace pcv
