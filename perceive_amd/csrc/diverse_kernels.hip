// diverse_kernels.hip — the two device steps of pcv_searcher_search_diverse (DESIGN.md §4 "Diverse results"): greedy maximal
// marginal relevance over the first `pool` entries of a query's ranked list, selected where the ranked lists live.
//
// collect  diverse_collect_kernel, after every pass: the pass's hits (rescore_select_kernel: p.out, best first, a short list's
//          hits in front) are appended to the query's pool — position, canonical score, id — and their rows are gathered out of the
//          blocked layout into the scratch, piece-major (scan.h, DiverseArgs::rows).  One workgroup takes 16 hits of one query
//          (row_gather.h: four rows in flight per wave).
// select   diverse_select_kernel, once per group of queries: one workgroup of 1024 threads per query makes the whole walk.
//          Thread t owns pool entries t, t + 1024, ... — at most four (PCV_MAX_DIVERSE_POOL = 4 x 1024), so what belongs to an
//          entry lives in its owner's REGISTERS: relevance, canonical |x|^2, the running redundancy `div`, picked or not.
//          Per step the row picked last is copied from the scratch into LDS, every thread runs the feature-order f64 chains of
//          its entries' rows against it (pair_sums: up to four independent chains a thread; the LDS row is read as a broadcast,
//          the scratch rows coalesced), finishes each cosine (finish_score) with the norms computed once in the same order,
//          folds it into div, forms m = fl(fl(lambda rel) - fl(mu div)) without contraction, and a workgroup argmax on
//          (m, lower rank) — shuffles inside a wave, 16 slots across the waves — picks the next row.  num_results x pool x dim
//          FMAs per query: no pool x pool matrix is ever formed.
// LDS plan: one f32 row of Dp features (32 KB at 8192-d, the widest row the searcher takes) and the 16 reduction slots, whatever
// the pool — div needs no LDS.  Launch bounds of 1024 leave 128 registers a thread; the four-chain form takes 121, without spills.
#include "device_access.h"
#include "row_gather.h"
#include "scan.h"

namespace pcv {
namespace {

constexpr int kDiverseThreads = 1024;
constexpr int kDiverseWaves = kDiverseThreads / 64;
constexpr int kCollectRows = 16;  // hits one collect workgroup gathers

__global__ __launch_bounds__(256) void diverse_collect_kernel(const ScanParams* __restrict__ pp, const DiverseArgs a) {
    const ScanParams& p = *pp;
    __shared__ uint64_t src[kCollectRows];
    __shared__ uint32_t n_found;
    const int q = blockIdx.x, tid = threadIdx.x, n_list = p.k, D4 = p.D4;
    const pcv_hit_dev* hits = p.out + (size_t)q * n_list;
    if (tid == 0) n_found = 0;
    __syncthreads();
    if (tid < n_list && gld(&hits[tid].pos) >= 0) atomicAdd(&n_found, 1u);  // (the hits of a short list come first)
    __syncthreads();
    const int room = min(a.pool, a.cap) - a.walked;
    const int n_new = min((int)n_found, max(room, 0));
    const int i0 = (int)blockIdx.y * kCollectRows;
    const int n = max(0, min(kCollectRows, n_new - i0));
    const size_t e0 = (size_t)a.walked + i0;
    if (tid < n) {
        pcv_hit_dev h;
        h.score = gld(&hits[i0 + tid].score);
        h.pos = gld(&hits[i0 + tid].pos);
        h.id = gld(&hits[i0 + tid].id);
        src[tid] = row_start(p, h.pos);
        a.entries[(size_t)q * a.cap + e0 + tid] = h;
    }
    __syncthreads();
    stage_rows(a.rows + (size_t)q * D4 * a.cap + e0, 1, (size_t)a.cap, src, n, D4, tid);
    if (blockIdx.y == 0 && tid == 0) {  // (the record is this thread's alone: the other workgroups of the query never read it)
        DistinctRec rec = a.rec[q];
        if (rec.flags == 0) {
            rec.examined = (uint32_t)(a.walked + n_new);
            if (n_new > 0) {
                rec.last_score = gld(&hits[n_new - 1].score);
                rec.last_pos = gld(&hits[n_new - 1].pos);
            }
            if (n_new < n_list) rec.flags = kDistinctEnd;  // a short list: the query has all the rows there are
            a.rec[q] = rec;
        }
        a.rec_host[q] = rec;
    }
}

// m = fl(fl(lambda rel) - fl(mu div)): three roundings, never a fused multiply-add
__device__ __forceinline__ double marginal(double lambda, double mu, double rel, double div) {
#pragma clang fp contract(off)
    const double x = lambda * rel;
    const double y = mu * div;
    return x - y;
}
// the certificate's bound: fl(fl(lambda rel_last) + fl(mu d0))
__device__ __forceinline__ double outside_bound(double lambda, double mu, double rel_last) {
#pragma clang fp contract(off)
    const double d0 = 1.0 + 0x1p-40;
    const double x = lambda * rel_last;
    const double y = mu * d0;
    return x + y;
}

struct DiverseLds {
    double red_m[kDiverseWaves];
    int32_t red_e[kDiverseWaves];
    double x_norm;
};

// One workgroup per query.  NU: pool entries a thread owns, ceil(pool / 1024).
template <int NU>
__global__ __launch_bounds__(kDiverseThreads) void diverse_select_kernel(const DiverseArgs a, int D, int D4, int metric) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    float4* xrow = (float4*)lds_raw;
    DiverseLds& s = *(DiverseLds*)(xrow + D4);
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t cap = (size_t)a.cap;
    DistinctRec rec = a.rec[q];
    const int P = min((int)rec.examined, a.pool);
    const int K = min(a.num_results, P);
    const pcv_hit_dev* entries = a.entries + (size_t)q * cap;
    const float4* rows = a.rows + (size_t)q * D4 * cap;
    const double lambda = a.lambda, mu = 1.0 - a.lambda;

    int e[NU];
    bool live[NU];
    const float4* yb[NU];
    double rel[NU], nrm[NU], div[NU];
    uint32_t picked = 0;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        e[u] = tid + kDiverseThreads * u;
        live[u] = e[u] < P;
        yb[u] = rows + min(e[u], max(P - 1, 0));
        rel[u] = live[u] ? relevance(metric, D, gld(&entries[e[u]].score)) : 0.0;
        nrm[u] = 0.0;
        div[u] = 0.0;
    }
    // canonical |x|^2 of every entry: the chain of the row with itself
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        if (live[u]) {
            const float4* y1[1] = {yb[u]};
            double n1[1];
            pair_sums<1>(yb[u], cap, y1, cap, D4, n1);
            nrm[u] = n1[0];
        }
    }
    bool all_above = true;
    const double bound = P > 0 ? outside_bound(lambda, mu, relevance(metric, D, gld(&entries[P - 1].score))) : 0.0;
    for (int t = 0; t < K; ++t) {
        double bm = -__builtin_inf();
        int be = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (live[u] && !(picked >> u & 1u)) {
                const double m = marginal(lambda, mu, rel[u], div[u]);
                if (better(m, e[u], bm, be)) bm = m, be = e[u];
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double om = __shfl_xor(bm, off);
            const int oe = __shfl_xor(be, off);
            if (better(om, oe, bm, be)) bm = om, be = oe;
        }
        if (lane == 0) s.red_m[wave] = bm, s.red_e[wave] = be;
        __syncthreads();
        bm = s.red_m[0], be = s.red_e[0];
#pragma unroll
        for (int w = 1; w < kDiverseWaves; ++w) {
            const double om = s.red_m[w];
            const int oe = s.red_e[w];
            if (better(om, oe, bm, be)) bm = om, be = oe;
        }
        // (K <= P: an entry not yet picked exists, and its m is finite — `be` is an entry)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (e[u] == be) {
                picked |= 1u << u;
                s.x_norm = nrm[u];
            }
        }
        if (tid == 0) {
            const size_t o = (size_t)q * kMaxK + t;
            a.out_id[o] = gld(&entries[be].id);
            a.out_score[o] = gld(&entries[be].score);
            a.out_marginal[o] = bm;
            a.out_rank[o] = be;
            all_above = all_above && bm > bound;
        }
        if (t + 1 == K) break;
        __syncthreads();  // (every thread has read the slots and the row of the step before)
        for (int f = tid; f < D4; f += kDiverseThreads) xrow[f] = gld4(rows + (size_t)f * cap + be);
        __syncthreads();
        if (live[0]) {  // (entries ascend with u: a thread without a first entry has none)
            double acc[NU];
            pair_sums<NU>(xrow, 1, yb, cap, D4, acc);
            const double xn = s.x_norm;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                double c = finish_score(PCV_METRIC_COSINE, acc[u], nrm[u], xn);
                if (!(c == c)) c = 0.0;  // a pair without a cosine counts as orthogonal
                if (t == 0 || c > div[u]) div[u] = c;
            }
        }
    }
    if (tid == 0) {
        rec.kept = (uint32_t)K;
        a.rec[q] = rec;
        a.rec_host[q] = rec;
        a.out_exact[q] = (P < a.pool || all_above) ? 1u : 0u;
    }
}

}  // namespace

void launch_diverse_collect(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DiverseArgs& a) {
    PCV_REQUIRE(p.B > 0 && p.k >= 1 && p.k <= kMaxK && p.nseg > 0 && a.walked >= 0 && a.walked + p.k <= a.pool && a.pool <= a.cap,
                "diverse collect: bad shape (%d queries, lists of %d behind %d of a pool of %d, room for %d)", p.B, p.k, a.walked, a.pool, a.cap);
    diverse_collect_kernel<<<dim3((unsigned)p.B, (unsigned)((p.k + kCollectRows - 1) / kCollectRows)), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

void launch_diverse_select(hipStream_t st, int B, int D, int D4, int metric, const DiverseArgs& a) {
    PCV_REQUIRE(B > 0 && a.num_results >= 1 && a.num_results <= kMaxK && a.pool >= a.num_results && a.pool <= a.cap &&
                    a.pool <= 4 * kDiverseThreads,
                "diverse select: bad shape (%d queries, %d results of a pool of %d, room for %d)", B, a.num_results, a.pool, a.cap);
    const size_t lds = (size_t)D4 * sizeof(float4) + sizeof(DiverseLds);
    if (lds > (size_t)64 * 1024) PCV_FAIL(PCV_ERR_UNSUPPORTED, "search_diverse: dimension %d is too large for the LDS row", D);
    switch ((a.pool + kDiverseThreads - 1) / kDiverseThreads) {
        case 1: diverse_select_kernel<1><<<B, kDiverseThreads, lds, st>>>(a, D, D4, metric); break;
        case 2: diverse_select_kernel<2><<<B, kDiverseThreads, lds, st>>>(a, D, D4, metric); break;
        case 3: diverse_select_kernel<3><<<B, kDiverseThreads, lds, st>>>(a, D, D4, metric); break;
        default: diverse_select_kernel<4><<<B, kDiverseThreads, lds, st>>>(a, D, D4, metric); break;
    }
    PCV_LAUNCHED();
}

}  // namespace pcv
