// compound_kernels.hip — the select step of pcv_searcher_search_compound (corpus.h "compound queries"; DESIGN.md §4 "Compound
// queries"): after every pass of the walk the hits of all the lists of a compound are candidates; a row met for the first time is
// scored under EVERY vector of its compound — its f32 row read once, found via row_start —, combined into m = fl(base - pen), merged
// with the rows kept so far (m descending, ties -> lower global position), and the certificate is tested.
//
// Nothing here depends on the order in which anything lands.  Whether a candidate is dropped as a repeat is a question about
// positions that are at rest behind a barrier (the kept rows, the candidates of the lists BEFORE its own: inside one list positions
// are distinct); a candidate's slot is the NUMBER of candidates and kept rows that order before it — after the repeats are dropped
// the positions are distinct, so the order is total and the slots are distinct whatever the timing —; the per-list counts are
// ballots, and every record is written by one thread.
// LDS plan: kMaxCompoundParts x kMaxK candidates and kMaxK kept rows, (m, position) each: 18 KB, whatever the dimension; the norms of
// the compound's vectors and the per-wave counts: under 300 bytes.  On top, in the dynamic region, the compound's W + A vectors
// (16 x 1.5 KB = 24 KB at 384-d) where that is at most kVectorLdsBytes; wider rows (16 vectors of more than 2048 features; a CU has
// 160 KB) read the vectors from global memory instead, every lane of a wave the same address.
#include "corpus.h"
#include "device_access.h"
#include "row_gather.h"
#include "scan.h"

namespace pcv {
namespace {

constexpr int kParts = kMaxCompoundParts;
constexpr int kVecs = 2 * kParts;      // wanted and avoided vectors of one compound at most
constexpr int kCand = kParts * kMaxK;  // candidates of one pass at most: one thread each
constexpr int64_t kNoPos = INT64_MAX;  // the position of an empty slot: it orders after every row there is
constexpr size_t kVectorLdsBytes = (size_t)128 << 10;
static_assert(kMaxK == 128 && kCand == 1024, "thread t is candidate t & 127 of list t >> 7");

// m = fl(base - pen), pen = fl(lambda * hinge): two roundings
__device__ __forceinline__ double combine(double base, double lambda, double hinge, double& pen) {
#pragma clang fp contract(off)
    pen = lambda * hinge;
    return base - pen;
}

// One workgroup per compound, kMaxK threads for each list of the widest compound of the group.  Thread t is candidate t & 127 of
// list t >> 7 (p.out, best first; the hits of a short list come first) AND, below kMaxK, kept row t of the state block.  Both are read
// into registers before the first barrier; what is written to the state block behind the last barrier but one overwrites only rows
// every thread has already read.
template <bool LDSVEC>
__global__ __launch_bounds__(kCand) void compound_select_kernel(const ScanParams* __restrict__ pp, const CompoundArgs a) {
    const ScanParams& p = *pp;
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];  // LDSVEC: [W + A][D4] pieces of the compound's vectors
    __shared__ double s_m[kCand + kMaxK];     // [0, kCand): the pass's candidates; [kCand, +kMaxK): the rows kept so far
    __shared__ int64_t s_pos[kCand + kMaxK];  // first the positions the repeats are found by (-1: none), then those of the order
    __shared__ double s_nq[kVecs];            // canonical |q|^2 of the compound's vectors
    __shared__ double s_last[kParts];         // relevance of the last entry walked in each list
    __shared__ int32_t s_wlive[kCand / 64], s_wnew[kCand / 64];  // per wave: hits of the pass; candidates that were scored
    __shared__ int32_t s_full;
    const int cq = blockIdx.x, t = threadIdx.x, nthreads = blockDim.x;
    const CompoundDesc d = a.desc[cq];
    const int W = d.n_want, NV = d.n_want + d.n_avoid, fq = d.first_query;
    const int n_list = p.k, K = a.num_results, D4 = p.D4;
    const DistinctRec rec = a.rec[fq];
    if (rec.flags != 0) {  // finished in an earlier pass: nothing of it changes
        if (t < W) a.rec_host[fq + t] = a.rec[fq + t];
        return;
    }
    const float4* want_v = (const float4*)p.qraw + (size_t)fq * D4;  // the pass's raw queries, zero padded
    const float4* avoid_v = (const float4*)a.avoid + (size_t)d.first_avoid * D4;
    float4* sv = (float4*)lds_raw;
    if constexpr (LDSVEC) {
        for (int i = t; i < NV * D4; i += nthreads) sv[i] = i < W * D4 ? gld4(want_v + i) : gld4(avoid_v + (i - W * D4));
    }
    if (t < NV) s_nq[t] = t < W ? gld(&a.want_norm[fq + t]) : gld(&a.avoid_norm[d.first_avoid + t - W]);
    if (t == 0) s_full = 0;
    // candidate i of list j
    const int j = t >> 7, i = t & (kMaxK - 1);
    pcv_hit_dev h;
    h.score = 0.0, h.pos = -1, h.id = -1;
    if (j < W && i < n_list) {
        const pcv_hit_dev* src = p.out + (size_t)(fq + j) * n_list + i;
        h.score = gld(&src->score), h.pos = gld(&src->pos), h.id = gld(&src->id);
    }
    bool live = h.pos >= 0;
    // kept row t
    const size_t o = (size_t)cq * kMaxK;
    const int nk0 = (int)rec.kept;
    const bool old = t < nk0;
    pcv_hit_dev oh;
    oh.score = -__builtin_inf(), oh.pos = kNoPos, oh.id = -1;
    double open = 0.0, opart[kParts];
#pragma unroll
    for (int u = 0; u < kParts; ++u) opart[u] = 0.0;
    if (old) {
        oh.score = gld(&a.kept[o + t].score), oh.pos = gld(&a.kept[o + t].pos), oh.id = gld(&a.kept[o + t].id);
        open = gld(&a.kept_pen[o + t]);
#pragma unroll
        for (int u = 0; u < kParts; ++u) opart[u] = gld(&a.kept_part[(o + t) * kParts + u]);
    }
    s_pos[t] = live ? h.pos : -1;
    if (t < kMaxK) s_pos[kCand + t] = old ? oh.pos : -1;
    const unsigned long long lmask = __ballot(live);
    if ((t & 63) == 0) s_wlive[t >> 6] = __popcll(lmask);
    __syncthreads();
    // a row that is kept already, or that a list before this one has brought in, is no candidate again
    if (live) {
        bool seen = false;
        for (int c = 0; c < nk0; ++c) seen = seen || s_pos[kCand + c] == h.pos;
        for (int c = 0; c < j * kMaxK; ++c) seen = seen || s_pos[c] == h.pos;
        live = !seen;
    }
    const uint64_t row = live ? row_start(p, h.pos) : 0;
    live = live && row != 0;
    // the canonical sums of the row with every vector of the compound, and with itself
    double c[kVecs], nx = 0.0;
#pragma unroll
    for (int u = 0; u < kVecs; ++u) c[u] = 0.0;
    if (live) {
        const float4* x = (const float4*)row;
        for (int f = 0; f < D4; ++f) {
            const float4 v = gld4(x + (size_t)f * 32);
            nx += (double)v.x * (double)v.x;
            nx += (double)v.y * (double)v.y;
            nx += (double)v.z * (double)v.z;
            nx += (double)v.w * (double)v.w;
#pragma unroll
            for (int u = 0; u < kVecs; ++u) {
                if (u < NV) {  // (the same in every thread of the workgroup)
                    float4 w;
                    if constexpr (LDSVEC)
                        w = sv[u * D4 + f];
                    else
                        w = u < W ? gld4(uniform_ptr(want_v + (size_t)u * D4) + f) : gld4(uniform_ptr(avoid_v + (size_t)(u - W) * D4) + f);
                    c[u] += (double)w.x * (double)v.x;
                    c[u] += (double)w.y * (double)v.y;
                    c[u] += (double)w.z * (double)v.z;
                    c[u] += (double)w.w * (double)v.w;
                }
            }
        }
    }
    const bool all = a.mode == PCV_COMPOUND_ALL;
    double base = all ? __builtin_inf() : -__builtin_inf(), hinge = 0.0;
#pragma unroll
    for (int u = 0; u < kVecs; ++u) {
        if (u < NV) {
            c[u] = finish_score(p.metric, c[u], nx, s_nq[u]);
            live = live && c[u] == c[u];  // NaN: the row has no score under this vector
            const double r = relevance(p.metric, p.D, c[u]);
            if (u < W)
                base = all ? (r < base ? r : base) : (r > base ? r : base);
            else
                hinge = r > hinge ? r : hinge;
        } else if (u < kParts) {
            c[u] = __builtin_nan("");
        }
    }
    double pen = 0.0;
    const double m = live ? combine(base, a.lambda, hinge, pen) : -__builtin_inf();
    const int64_t pos = live ? h.pos : kNoPos;
    const int n_live = j < W ? s_wlive[2 * j] + s_wlive[2 * j + 1] : 0;  // of this thread's list
    __syncthreads();  // (the positions the repeats were found by are read)
    s_m[t] = m, s_pos[t] = pos;
    if (t < kMaxK) s_m[kCand + t] = oh.score, s_pos[kCand + t] = oh.pos;
    const unsigned long long nmask = __ballot(live);
    if ((t & 63) == 0) s_wnew[t >> 6] = __popcll(nmask);
    if (j < W && i == n_live - 1) s_last[j] = relevance(p.metric, p.D, h.score);
    __syncthreads();
    // rank by counting: every candidate and kept row that orders before mine (an empty slot orders before nothing)
    int slot = 0, oslot = 0;
    for (int e = 0; e < W * kMaxK; ++e) {
        const double em = s_m[e];
        const int64_t ep = s_pos[e];
        slot += better(em, ep, m, pos) ? 1 : 0;
        oslot += better(em, ep, oh.score, oh.pos) ? 1 : 0;
    }
    for (int e = kCand; e < kCand + nk0; ++e) {
        const double em = s_m[e];
        const int64_t ep = s_pos[e];
        slot += better(em, ep, m, pos) ? 1 : 0;
        oslot += better(em, ep, oh.score, oh.pos) ? 1 : 0;
    }
    int n_new = 0, most = 0;
    bool ended = false;
    for (int w = 0; w < W; ++w) {
        const int n = s_wlive[2 * w] + s_wlive[2 * w + 1];
        n_new += s_wnew[2 * w] + s_wnew[2 * w + 1];
        most = max(most, n);
        ended = ended || n < n_list;  // a short list: the parts have listed every selectable row
    }
    const int n_kept = min(K, nk0 + n_new);
    // (slot < n_kept <= kMaxK: inside the compound's rows of the state block)
    if (live && slot < n_kept) {
        pcv_hit_dev nh;
        nh.score = m, nh.pos = h.pos, nh.id = h.id;
        a.kept[o + slot] = nh;
        gst(&a.kept_pen[o + slot], pen);
#pragma unroll
        for (int u = 0; u < kParts; ++u) gst(&a.kept_part[(o + slot) * kParts + u], c[u]);
    }
    if (old && oslot < n_kept && oslot != t) {
        a.kept[o + oslot] = oh;
        gst(&a.kept_pen[o + oslot], open);
#pragma unroll
        for (int u = 0; u < kParts; ++u) gst(&a.kept_part[(o + oslot) * kParts + u], opart[u]);
    }
    // the certificate: the owner of slot num_results - 1 tests its m against what a row met in no list can reach.  Strictly: an
    // unmet row with m == T may have the lower position.
    if (!ended) {
        double T = s_last[0];
#pragma unroll
        for (int w = 1; w < kParts; ++w)
            if (w < W) T = all ? (s_last[w] < T ? s_last[w] : T) : (s_last[w] > T ? s_last[w] : T);
        if ((live && slot == K - 1 && m > T) || (old && oslot == K - 1 && oh.score > T)) s_full = 1;
    }
    __syncthreads();
    if (j < W && i == max(n_live - 1, 0)) {  // the record of list j, by the thread of its last hit
        const DistinctRec mine = a.rec[fq + j];
        DistinctRec out;
        out.kept = (uint32_t)n_kept;
        out.examined = rec.examined + (uint32_t)most;
        out.flags = ended ? kDistinctEnd : (s_full ? kDistinctFull : 0u);
        out.pad = 0;
        out.last_score = n_live > 0 ? h.score : mine.last_score;
        out.last_pos = n_live > 0 ? h.pos : mine.last_pos;
        a.rec[fq + j] = out;
        a.rec_host[fq + j] = out;
    }
}

}  // namespace

void launch_compound_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const CompoundArgs& a) {
    PCV_REQUIRE(p.B > 0 && p.k >= 1 && p.k <= kMaxK && a.num_results >= 1 && a.num_results <= kMaxK && p.nseg > 0,
                "compound select: bad shape (%d queries, lists of %d, %d results)", p.B, p.k, a.num_results);
    PCV_REQUIRE(a.n_compounds >= 1 && a.n_compounds <= p.B && a.max_want >= 1 && a.max_want <= kParts && a.max_vectors >= a.max_want &&
                    a.max_vectors <= kVecs,
                "compound select: bad group (%d compounds, up to %d wanted and %d vectors each)", a.n_compounds, a.max_want, a.max_vectors);
    PCV_REQUIRE(a.mode == PCV_COMPOUND_ALL || a.mode == PCV_COMPOUND_ANY, "compound select: mode %d", a.mode);
    const size_t vec_bytes = (size_t)a.max_vectors * p.D4 * sizeof(float4);
    const unsigned threads = (unsigned)a.max_want * kMaxK;
    if (vec_bytes <= kVectorLdsBytes) {
        allow_dynamic_lds((const void*)compound_select_kernel<true>, vec_bytes);
        compound_select_kernel<true><<<a.n_compounds, threads, vec_bytes, st>>>(dp, a);
    } else {
        compound_select_kernel<false><<<a.n_compounds, threads, 0, st>>>(dp, a);
    }
    PCV_LAUNCHED();
}

}  // namespace pcv
