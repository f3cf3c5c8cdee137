// selfjoin_kernels.hip — the three steps of pcv_searcher_find_duplicates (DESIGN.md §4 "Duplicate pairs"): every pair of
// participating rows whose canonical cosine is at or above a threshold, exact, computed where the rows live.
//
//   1. selfjoin_prep_kernel     one thread per row: the canonical |x|^2 (f64, feature order) and rinv = 1/|x| in f32 (scan.h,
//                               SelfJoinArgs: 0 = the row takes no part).  Reads the corpus once.
//   2. selfjoin_screen_kernel   the 128-query bf16 scan with rows in the place of queries: a workgroup stages a tile of up to 128
//                               consecutive rows in LDS as bf16 (the layout scan_mfma_kernel uses for its query tile) and streams a
//                               span of the blocks at and after the tile's first block out of the blocked f32 layout, rounding a
//                               lane's 16-byte pieces to bf16 on the way — they are the A fragment of v_mfma_f32_32x32x16_bf16.
//                               s = acc * rinv_a * rinv_b; a pair with s >= threshold - margin (selfjoin_margin: a certified bound
//                               on |s - c|) and row a before row b is appended to one device list.  Only the upper triangle is
//                               computed.  Appends past the list's capacity are counted, not stored: the host repeats the launch
//                               once with the capacity the count asks for.
//   3. selfjoin_rescore_kernel  one thread per candidate: the canonical f64 cosine (pair_sums and finish_score, device_access.h —
//                               the arithmetic of distinct_select_kernel), kept iff c >= threshold.
#include "device_access.h"
#include "launch_rows.h"
#include "pair_screen.h"
#include "row_jobs.h"

namespace pcv {
namespace {

__global__ __launch_bounds__(256) void selfjoin_prep_kernel(const ScanParams* __restrict__ pp, const SelfJoinArgs a) {
    const ScanParams& p = *pp;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)p.total_blocks * 32) return;
    const RowRef r = row_ref(p, (uint32_t)i);
    float rinv = 0.0f;
    double n = 0.0;
    if (r.row < gld(&r.sg->nrows) && gld(&gld(&r.sg->scale)[r.row]) != 0.0f) {
        const float4* y[1] = {r.x};
        double acc[1];
        pair_sums<1>(r.x, y, p.D4, acc, 32);
        n = acc[0];
        if (n >= 0x1p-126 && n < __builtin_inf())  // (finish_score's condition for a cosine)
            rinv = (n >= 0x1p-40 && n <= 0x1p40) ? (float)(1.0 / sqrt(n)) : kRinvWild;
    }
    gst(&a.rinv[i], rinv);
    gst(&a.norm[i], n);
}

// The epilogue of the duplicate screen: a pair with s >= the screening threshold (or a wild row: every pair, scan.h) is listed; in a
// block of the tile's own only with row a before row b.
template <int NT>
struct JoinPolicy {
    const SelfJoinArgs& a;
    __device__ __forceinline__ void begin(uint32_t, int) {}
    __device__ __forceinline__ void prefetch(uint32_t, int, int) {}
    __device__ __forceinline__ void end(const float (&)[NT], int, int) {}
    __device__ __forceinline__ void block(const f32x16 (&acc)[NT], const float (&ra)[NT], const f32x4 (&rb)[4], const PairWhere& at) {
        const float thr = a.screen_threshold;
        const bool diagonal = at.gb < at.tb0 + NT;  // the block is one of the tile's own: row a before row b only
        auto passes = [&](int t, int i) -> bool {
            const float rbi = rb[i >> 2][i & 3];
            const float s = acc[t][i] * ra[t] * rbi;
            bool ok = (ra[t] > 0.0f && rbi > 0.0f) ? s >= thr : (ra[t] != 0.0f && rbi != 0.0f);
            if (diagonal) ok = ok && at.owner_row(t) < at.partner_row(i);
            return ok;
        };
        bool any = false;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) any |= passes(t, i);
        if (!__any(any)) return;  // (the common case)
        uint32_t mask[NT];
        uint32_t n = 0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            mask[t] = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) mask[t] |= passes(t, i) ? (1u << i) : 0u;
            n += (uint32_t)__builtin_popcount(mask[t]);
        }
        if (n) {
            unsigned long long k = g_atomic_add64(&a.counters[0], n);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                uint32_t m = mask[t];
                while (m) {
                    const int i = __builtin_ctz(m);
                    m &= m - 1;
                    if (k < a.cand_cap) gst(&a.cand[k], ((uint64_t)at.owner_row(t) << 32) | at.partner_row(i));
                    ++k;
                }
            }
        }
    }
};

// grid: x = tile (tile_blocks = NT consecutive blocks), y = span: the blocks [tile's first + y * span_blocks, + span_blocks) of the
// launch, cut at its end.  A (tile, span) that starts behind the end has nothing to do.  Consecutive workgroups stream nearly the
// same blocks, NT blocks apart: what one brings into the L2 the next ones find there.  Wave w takes the blocks first + w,
// first + w + kScreenWaves, ...  Staging, stream and accumulator layout: pair_screen.h.
template <int NT>
__global__ __launch_bounds__(kScreenWaves * 64) void selfjoin_screen_kernel(const ScanParams* __restrict__ pp, const SelfJoinArgs a) {
    const ScanParams& p = *pp;
    extern __shared__ uint4 lq[];
    __shared__ const float4* tbase[NT];
    const uint32_t TB = p.total_blocks;
    const uint32_t tb0 = blockIdx.x * NT;
    const uint64_t first = (uint64_t)tb0 + (uint64_t)blockIdx.y * a.span_blocks;
    if (first >= TB) return;  // (the whole workgroup)
    const uint32_t b0 = (uint32_t)first;
    const uint32_t b1 = (uint32_t)min((uint64_t)TB, first + a.span_blocks);
    pair_stage_tile<NT>(p, lq, tbase, tb0);
    const uint32_t wave = uniform(threadIdx.x >> 6);
    if (b0 + wave >= b1) return;
    JoinPolicy<NT> pol{a};
    pair_stream<NT>(p, lq, a.rinv, tb0, b0 + wave, b1, kScreenWaves, pol);
}

__global__ __launch_bounds__(256) void selfjoin_rescore_kernel(const ScanParams* __restrict__ pp, const SelfJoinArgs a) {
    const ScanParams& p = *pp;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_cand) return;
    const uint64_t cd = gld(&a.cand[i]);
    const uint32_t la = (uint32_t)(cd >> 32), lb = (uint32_t)cd;
    const RowRef ra = row_ref(p, la), rb = row_ref(p, lb);
    const float4* y[1] = {rb.x};
    double acc[1];
    pair_sums<1>(ra.x, y, p.D4, acc, 32);
    const double cc = finish_score(PCV_METRIC_COSINE, acc[0], gld(&a.norm[la]), gld(&a.norm[lb]));
    if (!(cc >= a.threshold)) return;
    if (a.grp != nullptr) {  // find_duplicates_grouped: a pair of siblings (the 64-bit keys, row_jobs.h PairGroups) is counted, not emitted
        const int64_t ga = gld(&a.grp[la]);
        if (ga >= 0 && ga == gld(&a.grp[lb])) {
            (void)g_atomic_add64(a.skipped, 1ull);
            return;
        }
    }
    const unsigned long long at = g_atomic_add64(&a.counters[1], 1ull);
    if (at >= a.pair_cap) return;
    const int64_t pa = gld(&ra.sg->pos0) + (int64_t)ra.row, pb = gld(&rb.sg->pos0) + (int64_t)rb.row;
    const int64_t ia = row_id(ra), ib = row_id(rb);
    const bool fwd = pa < pb;
    DupPair* out = &a.pairs[at];
    gst(&out->c, cc);
    gst(&out->pos_a, fwd ? pa : pb);
    gst(&out->pos_b, fwd ? pb : pa);
    gst(&out->id_a, fwd ? ia : ib);
    gst(&out->id_b, fwd ? ib : ia);
}

}  // namespace

// |s - c| for s = fl(fl(acc ra) rb) (DESIGN.md §4 "Duplicate pairs"), relative to |a||b| = 1 after the two rinv factors:
//   two bf16 operand roundings, u = 2^-8 each:   u (2 + u)                      = 0.0078278
//   f32 accumulation over Dp terms, any order:   eps32 (1 + u)^2,  eps32 = (Dp + 16) 2^-23 as for the scans
//   two rinv roundings and two multiplies:       4 * 2^-24 (1 + the above), and what f64 leaves of the canonical sums: all in 1e-6
float selfjoin_margin(int Dp) { return 0.00783f + 1.02f * ((float)(Dp + 16) * 1.2e-7f) + 1e-6f; }

void launch_selfjoin_prep(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SelfJoinArgs& a) {
    if (p.total_blocks == 0) return;
    selfjoin_prep_kernel<<<cdiv64((int64_t)p.total_blocks * 32, 256), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

void launch_selfjoin_screen(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SelfJoinArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t NT = a.tile_blocks;
    PCV_REQUIRE((NT == 1 || NT == 2 || NT == 4) && a.span_blocks >= NT, "self-join screen: bad tile (%u blocks, spans of %u)", NT, a.span_blocks);
    const size_t lds = (size_t)NT * 32 * p.D4 * 4 * sizeof(uint16_t);
    const unsigned tiles = (p.total_blocks + NT - 1) / NT;
    const unsigned spans = (p.total_blocks + a.span_blocks - 1) / a.span_blocks;
    PCV_REQUIRE(spans <= 65535u, "self-join screen: %u spans", spans);
    const dim3 grid(tiles, spans);
#define PCV_JOIN(N)                                                        \
    allow_dynamic_lds((const void*)selfjoin_screen_kernel<N>, lds);        \
    selfjoin_screen_kernel<N><<<grid, kScreenWaves * 64, lds, st>>>(dp, a);
    if (NT == 4) {
        PCV_JOIN(4)
    } else if (NT == 2) {
        PCV_JOIN(2)
    } else {
        PCV_JOIN(1)
    }
#undef PCV_JOIN
    PCV_LAUNCHED();
}

void launch_selfjoin_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SelfJoinArgs& a) {
    if (a.n_cand == 0) return;
    selfjoin_rescore_kernel<<<cdiv64((int64_t)a.n_cand, 256), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

}  // namespace pcv
