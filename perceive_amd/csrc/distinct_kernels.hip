// distinct_kernels.hip — the select step of pcv_searcher_search_distinct (DESIGN.md §4 "Distinct results"): rows compared with
// rows, where the ranked lists live.
//
// After each pass of at most kMaxK ranked hits per query (rescore_select_kernel: p.out), one workgroup per query walks the
// pass's hits best first against the rows it kept in earlier passes and among themselves:
//     kept(row)  iff  cos(row, j) < threshold for every kept row j,
// cos the canonical cosine of the two stored f32 rows — f64, products exact, sums in feature order, finished by finish_score
// (device_access.h: the arithmetic rescore_select_kernel uses for query against row, and the only copy of it).  The cosine is
// symmetric bit for bit: the products commute, both sums run over the same features in the same order, and so does the product
// of the two roots.
//
// The hits are taken R at a time (a "chunk"; R = 32 at 384-d), so that no pair is computed that the walk cannot ask for:
//   1. the chunk's rows are gathered out of the blocked layout into LDS tile A (row pitch D4 + 1 pieces: a lane's 16-byte reads
//      of R different rows fall into different banks);
//   2. tile A against itself: 256 threads, thread (a, b-group) runs up to four feature-order chains at once — row a against rows
//      b, b + G, ... — each an f64 FMA chain over the row (the product of two f32 is exact in f64, so fma(x, y, acc) IS
//      acc + x * y rounded once).  The diagonal (a, a) is the row's own |x|^2, in the canonical order: no separate norm loop;
//   3. tile A against the kept rows, R at a time through LDS tile B (the rows kept in earlier chunks of this pass included);
//   4. every pair at or above the threshold sets a bit — row a against kept row j, row a against chunk row b < a —, and one thread
//      walks the chunk over the bit matrix: a row with a bit among the kept rows is dropped and counted for the lowest such row
//      (the best ranked), any other row is kept.  The walk stops right after the num_results-th kept row.
// 128 rows of 384 f32 are 192 KB and the kept rows as many again: the tiles are what fits the 160 KB of a CU (two tiles of
// 32 rows: 97 KB at 384-d; 2 rows a tile at 8192-d).
#include "device_access.h"
#include "row_gather.h"
#include "scan.h"

namespace pcv {
namespace {

constexpr int kDistinctRows = 32;  // most rows of an LDS tile (the chunk's bit matrix has 32-bit rows)

// LDS behind the two tiles (all of it in the dynamic region, every offset a multiple of 16)
struct DistinctLds {
    double a_norm[kDistinctRows];        // canonical |x|^2 of the chunk's rows
    uint64_t a_src[kDistinctRows];       // where each starts in the blocked layout (0: not found — compared as a zero row)
    uint32_t a_old[kDistinctRows][4];    // bit j: duplicate of kept row j
    uint32_t a_in[kDistinctRows];        // bit b: duplicate of chunk row b < a
    double k_norm[kMaxK];                // the kept rows: |x|^2, start, dropped rows counted for each
    uint64_t k_src[kMaxK];
    int32_t k_sim[kMaxK];
    uint32_t n_new, kept, examined, flags;
    double last_score;
    int64_t last_pos;
};

// (where a hit's row starts in the blocked layout and the gather into a tile: row_start / stage_rows, row_gather.h)
// (the feature-order f64 sums of a row of tile X with rows of tile Y: pair_sums, device_access.h)
// One workgroup per query.  R: rows of a tile, a power of two <= kDistinctRows; NU: chains a thread runs (R * R / 256, at least 1).
template <int NU>
__global__ __launch_bounds__(256) void distinct_select_kernel(const ScanParams* __restrict__ pp, const DistinctArgs a, int R, int logR) {
    const ScanParams& p = *pp;
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int D4 = p.D4, W = D4 + 1, n_list = p.k;
    float4* tA = (float4*)lds_raw;
    float4* tB = tA + (size_t)R * W;
    DistinctLds& s = *(DistinctLds*)(tB + (size_t)R * W);
    const DistinctRec rec = a.rec[q];
    if (rec.flags != 0) {  // finished in an earlier pass: nothing of it changes
        if (tid == 0) a.rec_host[q] = rec;
        return;
    }
    const pcv_hit_dev* hits = p.out + (size_t)q * n_list;
    pcv_hit_dev* kept = a.kept + (size_t)q * kMaxK;
    if (tid == 0) {
        s.n_new = 0;
        s.kept = rec.kept;
        s.examined = rec.examined;
        s.flags = 0;
        s.last_score = rec.last_score;
        s.last_pos = rec.last_pos;
    }
    __syncthreads();
    if (tid < n_list && gld(&hits[tid].pos) >= 0) atomicAdd(&s.n_new, 1u);  // (the hits of a short list come first)
    if (tid < (int)rec.kept) {
        s.k_norm[tid] = a.kept_norm[(size_t)q * kMaxK + tid];
        s.k_src[tid] = row_start(p, gld(&kept[tid].pos));
        s.k_sim[tid] = a.similar[(size_t)q * kMaxK + tid];
    }
    __syncthreads();
    const int n_new = (int)s.n_new;
    const int ra = tid & (R - 1), g = tid >> logR, G = 256 >> logR;  // this thread's row of tile A; its rows of tile Y: g + G u
    const float4* xa = tA + (size_t)ra * W;
    for (int c0 = 0; c0 < n_new; c0 += R) {
        const int nA = min(R, n_new - c0);
        const int nk0 = (int)s.kept;  // (same in every thread: the walk of the chunk before ended behind a barrier)
        if (tid < nA) s.a_src[tid] = row_start(p, gld(&hits[c0 + tid].pos));
        if (tid < kDistinctRows) {
            s.a_in[tid] = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) s.a_old[tid][w] = 0;
        }
        __syncthreads();
        stage_rows(tA, s.a_src, nA, D4, tid);
        __syncthreads();
        double acc[NU];
        {  // tile A against itself; the diagonal is |x|^2
            const float4* yb[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) yb[u] = tA + (size_t)min(g + G * u, R - 1) * W;
            const bool live = ra < nA && g < R;
            if (live) pair_sums<NU>(xa, yb, D4, acc);
#pragma unroll
            for (int u = 0; u < NU; ++u)
                if (live && g + G * u == ra) s.a_norm[ra] = acc[u];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int b = g + G * u;
                if (live && b < ra) {
                    const double c = finish_score(PCV_METRIC_COSINE, acc[u], s.a_norm[b], s.a_norm[ra]);
                    if (c >= a.threshold) atomicOr(&s.a_in[ra], 1u << b);
                }
            }
        }
        for (int t0 = 0; t0 < nk0; t0 += R) {  // ... against the kept rows
            const int nB = min(R, nk0 - t0);
            __syncthreads();  // (tile B's readers of the round before are through)
            stage_rows(tB, s.k_src + t0, nB, D4, tid);
            __syncthreads();
            const float4* yb[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) yb[u] = tB + (size_t)min(g + G * u, R - 1) * W;
            // (a wave whose rows of tile B are all behind nB has nothing to do)
            if (ra < nA && g < nB) {
                pair_sums<NU>(xa, yb, D4, acc);
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int b = g + G * u;
                    if (b < nB) {
                        const int j = t0 + b;
                        const double c = finish_score(PCV_METRIC_COSINE, acc[u], s.k_norm[j], s.a_norm[ra]);
                        if (c >= a.threshold) atomicOr(&s.a_old[ra][j >> 5], 1u << (j & 31));
                    }
                }
            }
        }
        __syncthreads();
        if (tid == 0) {  // the walk of the chunk
            uint32_t in_kept = 0;  // chunk rows kept; they follow the nk0 older ones in order
            int nk = nk0;
            uint32_t ex = s.examined;
            bool full = false;
            for (int i = 0; i < nA && !full; ++i) {
                const pcv_hit_dev h = hits[c0 + i];
                ++ex;
                s.last_score = h.score;
                s.last_pos = h.pos;
                int j = -1;
                for (int w = 0; w < 4 && j < 0; ++w)
                    if (s.a_old[i][w]) j = 32 * w + __builtin_ctz(s.a_old[i][w]);
                const uint32_t m = s.a_in[i] & in_kept;
                if (j < 0 && m) j = nk0 + __builtin_popcount(in_kept & ((1u << __builtin_ctz(m)) - 1u));
                if (j >= 0) {
                    s.k_sim[j] += 1;
                } else {
                    s.k_norm[nk] = s.a_norm[i];
                    s.k_src[nk] = s.a_src[i];
                    s.k_sim[nk] = 0;
                    kept[nk] = h;
                    in_kept |= 1u << i;
                    ++nk;
                    full = nk >= a.num_results;
                }
            }
            s.kept = (uint32_t)nk;
            s.examined = ex;
            if (full) s.flags = kDistinctFull;
        }
        __syncthreads();
        if (s.flags != 0) break;  // (same in every thread)
    }
    const int nk = (int)s.kept;
    if (tid < nk) {
        a.kept_norm[(size_t)q * kMaxK + tid] = s.k_norm[tid];
        a.similar[(size_t)q * kMaxK + tid] = s.k_sim[tid];
    }
    if (tid == 0) {
        DistinctRec out;
        out.kept = s.kept;
        out.examined = s.examined;
        out.flags = s.flags ? s.flags : (n_new < n_list ? kDistinctEnd : 0u);  // a short list: the query has all the rows there are
        out.pad = 0;
        out.last_score = s.last_score;
        out.last_pos = s.last_pos;
        a.rec[q] = out;
        a.rec_host[q] = out;
    }
}

}  // namespace

void launch_distinct_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DistinctArgs& a) {
    PCV_REQUIRE(p.B > 0 && p.k >= 1 && p.k <= kMaxK && a.num_results >= 1 && a.num_results <= kMaxK && p.nseg > 0,
                "distinct select: bad shape (%d queries, lists of %d, %d results)", p.B, p.k, a.num_results);
    const size_t row_bytes = ((size_t)p.D4 + 1) * sizeof(float4);
    int R = kDistinctRows, logR = 5;
    while (R > 1 && 2 * (size_t)R * row_bytes + sizeof(DistinctLds) > (size_t)150 * 1024) R >>= 1, --logR;
    const size_t lds = 2 * (size_t)R * row_bytes + sizeof(DistinctLds);
    if (lds > (size_t)158 * 1024) PCV_FAIL(PCV_ERR_UNSUPPORTED, "search_distinct: dimension %d is too large for the LDS tiles", p.D);
    if (R == kDistinctRows) {
        allow_dynamic_lds((const void*)distinct_select_kernel<4>, lds);
        distinct_select_kernel<4><<<p.B, 256, lds, st>>>(dp, a, R, logR);
    } else {
        allow_dynamic_lds((const void*)distinct_select_kernel<1>, lds);
        distinct_select_kernel<1><<<p.B, 256, lds, st>>>(dp, a, R, logR);
    }
    PCV_LAUNCHED();
}

}  // namespace pcv
