// boost_kernels.hip — the select step of pcv_searcher_search_boosted (corpus.h "boosted results"; DESIGN.md §4 "Boosted results"):
// after every pass of the walk the pass's hits are re-ranked, together with the rows kept so far, under the boosted score
// m = fl(rel + boost(value of the row's id)), ties -> lower rank in the list, and the certificate is tested.
//
// Nothing here depends on the order in which anything lands: the value table is only READ (plain loads of a table at rest: the
// owner's lock is held around the call), a candidate's slot is the NUMBER of candidates that order before it — the order
// (m descending, rank ascending) is total over distinct ranks, so the slots are distinct whatever the timing —, and the record is
// written by one thread.
// LDS plan: 2 x kMaxK candidates (m: 2 KB, rank: 1 KB) and the relevance of the pass's kMaxK hits (1 KB), whatever the dimension.
#include "corpus.h"
#include "device_access.h"
#include "scan.h"
#include "value_table.h"

namespace pcv {
namespace {

typedef unsigned long long u64;

constexpr int32_t kNoRank = 0x7fffffff;  // the rank of an empty candidate slot: it orders after every candidate there is

// boost(v) as perceive_hip.h defines it.  The knots are walked with constant indices (the loop is unrolled): a kernel argument
// indexed at run time would go through scratch memory.
__device__ __forceinline__ double boost_of(const pcv_boost& k, int64_t v) {
#pragma clang fp contract(off)
    if (v == kNoValue) return k.unset_boost;
    // the last knot at or below v, the knot behind it, and the last knot of all
    int64_t v0 = k.knot_values[0], v1 = v0, vn = v0;
    double b0 = k.knot_boosts[0], b1 = b0, bn = b0;
#pragma unroll
    for (int j = 1; j < (int)PCV_MAX_BOOST_KNOTS; ++j) {
        const bool have = j < k.n_knots;
        const bool below = have && k.knot_values[j - 1] <= v;  // knot j - 1 is at or below v and has knot j behind it
        v0 = below ? k.knot_values[j - 1] : v0;
        b0 = below ? k.knot_boosts[j - 1] : b0;
        v1 = below ? k.knot_values[j] : v1;
        b1 = below ? k.knot_boosts[j] : b1;
        vn = have ? k.knot_values[j] : vn;
        bn = have ? k.knot_boosts[j] : bn;
    }
    if (v <= k.knot_values[0]) return k.knot_boosts[0];
    if (v >= vn) return bn;
    // (here n_knots >= 2 and v0 <= v < v1)
    const double num = (double)((u64)v - (u64)v0);
    const double den = (double)((u64)v1 - (u64)v0);
    const double t = num / den;
    const double d = b1 - b0;
    const double p = t * d;
    double b = b0 + p;
    const double lo = b0 < b1 ? b0 : b1, hi = b0 < b1 ? b1 : b0;
    b = b >= lo ? b : lo;
    b = b <= hi ? b : hi;
    return b;
}

__device__ __forceinline__ double add_boost(double rel, double b) {
#pragma clang fp contract(off)
    return rel + b;
}

// does candidate (ma, ra) order before (mb, rb)?
__device__ __forceinline__ bool before(double ma, int32_t ra, double mb, int32_t rb) { return ma > mb || (ma == mb && ra < rb); }

// One workgroup of kMaxK threads per query, thread t for hit t of the pass's list (p.out, best first; the hits of a short list come
// first) AND for kept row t of the state block.  Both are read into registers before the first barrier; the slots come from LDS;
// what is written to the state block after the barrier overwrites only rows every thread has already read.
__global__ __launch_bounds__(kMaxK) void boost_select_kernel(const ScanParams* __restrict__ pp, const BoostArgs a) {
    const ScanParams& p = *pp;
    __shared__ double s_m[2 * kMaxK];      // [0, kMaxK): the pass's hits; [kMaxK, 2 kMaxK): the rows kept so far
    __shared__ int32_t s_rank[2 * kMaxK];  // kNoRank: no candidate
    __shared__ double s_rel[kMaxK];        // relevance of the pass's hits
    __shared__ u64 s_live[kMaxK / 64];
    __shared__ int32_t s_full;
    const int q = blockIdx.x, t = threadIdx.x, n_list = p.k, K = a.num_results;
    const DistinctRec rec = a.rec[q];
    if (rec.flags != 0) {  // finished in an earlier pass: nothing of it changes
        if (t == 0) a.rec_host[q] = rec;
        return;
    }
    const size_t o = (size_t)q * kMaxK;
    const int nk0 = (int)rec.kept;
    // the pass's hit t
    pcv_hit_dev h;
    h.score = 0.0, h.pos = -1, h.id = -1;
    if (t < n_list) {
        const pcv_hit_dev* src = p.out + (size_t)q * n_list + t;
        h.score = gld(&src->score), h.pos = gld(&src->pos), h.id = gld(&src->id);
    }
    const bool live = h.pos >= 0;
    const int64_t v = live ? value_of(a.table, h.id) : kNoValue;
    const double rel = live ? relevance(p.metric, p.D, h.score) : 0.0;
    const double m = live ? add_boost(rel, boost_of(a.boost, v)) : -__builtin_inf();
    const int32_t rank = live ? (int32_t)rec.examined + t : kNoRank;
    // kept row t
    const bool old = t < nk0;
    pcv_hit_dev oh;
    oh.score = 0.0, oh.pos = -1, oh.id = -1;
    double om = -__builtin_inf();
    int64_t ov = kNoValue;
    int32_t orank = kNoRank;
    if (old) {
        oh.score = gld(&a.kept[o + t].score), oh.pos = gld(&a.kept[o + t].pos), oh.id = gld(&a.kept[o + t].id);
        om = gld(&a.kept_m[o + t]);
        ov = gld(&a.kept_value[o + t]);
        orank = gld(&a.kept_rank[o + t]);
    }
    s_m[t] = m, s_rank[t] = rank, s_rel[t] = rel;
    s_m[kMaxK + t] = om, s_rank[kMaxK + t] = orank;
    const u64 lmask = __ballot(live);
    if ((t & 63) == 0) s_live[t >> 6] = lmask;
    if (t == 0) s_full = 0;
    __syncthreads();
    int n_live = 0;
#pragma unroll
    for (int w = 0; w < kMaxK / 64; ++w) n_live += __popcll(s_live[w]);
    // rank by counting: every candidate that orders before mine (an empty slot orders before nothing: m = -inf, rank = kNoRank)
    int slot = 0, oslot = 0;
    for (int c = 0; c < 2 * kMaxK; ++c) {
        const double cm = s_m[c];
        const int32_t cr = s_rank[c];
        slot += before(cm, cr, m, rank) ? 1 : 0;
        oslot += before(cm, cr, om, orank) ? 1 : 0;
    }
    const int n_kept = min(K, nk0 + n_live);
    // (slot < n_kept <= kMaxK: inside the query's rows of the state block)
    if (live && slot < n_kept) {
        a.kept[o + slot] = h;
        gst(&a.kept_m[o + slot], m);
        gst(&a.kept_value[o + slot], v);
        gst(&a.kept_rank[o + slot], rank);
    }
    if (old && oslot < n_kept && oslot != t) {
        a.kept[o + oslot] = oh;
        gst(&a.kept_m[o + oslot], om);
        gst(&a.kept_value[o + oslot], ov);
        gst(&a.kept_rank[o + oslot], orank);
    }
    // the certificate: the owner of slot num_results - 1 tests its m against what a row behind the last examined entry can reach
    if (n_live > 0) {
        const double bound = add_boost(s_rel[n_live - 1], a.b_max);
        if ((live && slot == K - 1 && m >= bound) || (old && oslot == K - 1 && om >= bound)) s_full = 1;
    }
    __syncthreads();
    if (t == max(n_live - 1, 0)) {
        DistinctRec out;
        out.kept = (uint32_t)n_kept;
        out.examined = rec.examined + (uint32_t)n_live;
        out.flags = n_live < n_list ? kDistinctEnd : (s_full ? kDistinctFull : 0u);  // a short list: the query has all the rows there are
        out.pad = 0;
        out.last_score = n_live > 0 ? h.score : rec.last_score;
        out.last_pos = n_live > 0 ? h.pos : rec.last_pos;
        a.rec[q] = out;
        a.rec_host[q] = out;
    }
}

}  // namespace

void launch_boost_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const BoostArgs& a) {
    PCV_REQUIRE(p.B > 0 && p.k >= 1 && p.k <= kMaxK && a.num_results >= 1 && a.num_results <= kMaxK,
                "boost select: bad shape (%d queries, lists of %d, %d results)", p.B, p.k, a.num_results);
    PCV_REQUIRE(a.table.keys == nullptr || (a.table.mask & (a.table.mask + 1)) == 0, "boost select: mask %#x", a.table.mask);
    PCV_REQUIRE(a.boost.n_knots >= 1 && a.boost.n_knots <= (int)PCV_MAX_BOOST_KNOTS, "boost select: %d knots", a.boost.n_knots);
    boost_select_kernel<<<p.B, kMaxK, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

}  // namespace pcv
