// seed_kernels.hip — the steps of pcv_searcher_seeds (DESIGN.md §4 "Seed items"): k stored rows picked one after the other, each by
// the integer weights the picks before it leave (k-means++ draw, or farthest first), exact, computed where the rows live.
//
//   0. selfjoin_prep_kernel   (selfjoin_kernels.hip, unchanged) the canonical |x|^2 per launch row; rinv == 0: the row takes no part.
//   1. seed_begin_kernel      one thread per launch row: cover = none, and the partials of step 0 (every participating row weighs 1).
//   2. seed_cover_kernel      one thread per launch row, the hot path: the canonical cosine of the row with the last pick
//                             (pair_sums and finish_score, device_access.h — the arithmetic of every other f64 decision), cover =
//                             max(cover, c), the row's weight, and per workgroup the sum of the weights and the best row.  A
//                             workgroup owns kSeedSpanRows consecutive launch rows: the partials are in position order.
//   3. seed_pick_kernel       one workgroup: the total T of the partials; T == 0 ends the call.  Farthest first reduces the partial
//                             bests; k-means++ draws t = seed_draw(seed, step, T), finds the span whose prefix range holds t by a scan
//                             of the partials and the row inside it by a scan of the span's weights, recomputed from cover.  It leaves
//                             the pick's launch row for the next cover step and writes the step's four outputs.
// Steps 2 and 3 are queued k - 1 and k times; nothing comes to the host in between.  The weights are integers, so T and every
// prefix sum are the same in any order of addition: the pick does not depend on how the rows are cut into workgroups.
#include "device_access.h"
#include "launch_rows.h"
#include "row_jobs.h"

namespace pcv {
namespace {

constexpr int kSeedWaves = kSeedSpanRows / 64;
constexpr uint32_t kNoRow = 0xffffffffu;

// (weight descending, launch row ascending): x comes before y.  Weight 0 with kNoRow: none.
__device__ __forceinline__ bool seed_before(unsigned long long wx, uint32_t rx, unsigned long long wy, uint32_t ry) {
    return wx > wy || (wx == wy && rx < ry);
}

__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int off) {
    const uint32_t lo = __shfl_up((uint32_t)v, off), hi = __shfl_up((uint32_t)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}

// What the threads of a workgroup share in LDS for the two collectives below.
struct SeedShared {
    unsigned long long sum[kSeedWaves];
    unsigned long long w[kSeedWaves];
    uint32_t row[kSeedWaves];
};

// The workgroup's sum of `sum` and its best (w, row); every thread receives all three.
__device__ __forceinline__ void seed_reduce(SeedShared& sh, unsigned long long& sum, unsigned long long& w, uint32_t& row) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        sum += shfl_xor_u64(sum, off);
        const unsigned long long ow = shfl_xor_u64(w, off);
        const uint32_t orow = __shfl_xor(row, off);
        if (seed_before(ow, orow, w, row)) {
            w = ow;
            row = orow;
        }
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();  // (the values of the collective before this one have been read)
    if ((threadIdx.x & 63) == 0) {
        sh.sum[wave] = sum;
        sh.w[wave] = w;
        sh.row[wave] = row;
    }
    __syncthreads();
    sum = 0;
    w = 0;
    row = kNoRow;
#pragma unroll
    for (int i = 0; i < kSeedWaves; ++i) {
        sum += sh.sum[i];
        if (seed_before(sh.w[i], sh.row[i], w, row)) {
            w = sh.w[i];
            row = sh.row[i];
        }
    }
}

// Inclusive prefix sum of v over the workgroup's threads, in thread order.
__device__ __forceinline__ unsigned long long seed_scan(SeedShared& sh, unsigned long long v) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = shfl_up_u64(v, off);
        if (lane >= off) v += o;
    }
    __syncthreads();
    if (lane == 63) sh.sum[wave] = v;
    __syncthreads();
    unsigned long long before = 0;
#pragma unroll
    for (int i = 0; i < kSeedWaves; ++i) before += i < wave ? sh.sum[i] : 0ull;
    return v + before;
}

__device__ __forceinline__ int64_t seed_id_of(const RowRef& r) {
    const int64_t* ids = gld(&r.sg->ids);
    return ids ? gld(&ids[r.row]) : gld(&r.sg->id0) + (int64_t)r.row;
}

__device__ __forceinline__ void seed_store_part(const SeedArgs& a, unsigned long long sum, unsigned long long w, uint32_t row) {
    SeedPart* out = &a.part[blockIdx.x];
    gst(&out->sum, sum);
    gst(&out->w, w);
    gst(&out->row, row);
}

__global__ __launch_bounds__(kSeedSpanRows) void seed_begin_kernel(const ScanParams* __restrict__ pp, const SeedArgs a) {
    const ScanParams& p = *pp;
    __shared__ SeedShared sh;
    const uint64_t i = (uint64_t)blockIdx.x * kSeedSpanRows + threadIdx.x;
    unsigned long long sum = 0, w = 0;
    uint32_t row = kNoRow;
    if (i < (uint64_t)p.total_blocks * 32) {
        gst(&a.cover[i], -__builtin_inf());
        if (gld(&a.rinv[i]) != 0.0f) {
            sum = 1;
            if (!a.has_first || seed_id_of(row_ref(p, (uint32_t)i)) == a.first_id) {  // (with a first id, the best of step 0 is its first row)
                w = 1;
                row = (uint32_t)i;
            }
        }
    }
    seed_reduce(sh, sum, w, row);
    if (threadIdx.x == 0) seed_store_part(a, sum, w, row);
}

__global__ __launch_bounds__(kSeedSpanRows) void seed_cover_kernel(const ScanParams* __restrict__ pp, const SeedArgs a) {
    const ScanParams& p = *pp;
    __shared__ SeedShared sh;
    if (gld(&a.state->done)) return;  // (the whole grid)
    const uint32_t centre = uniform(gld(&a.state->centre));
    const float4* cx = uniform_ptr(row_ref(p, centre).x);
    const double nc = gld(&a.norm[centre]);
    const uint64_t i = (uint64_t)blockIdx.x * kSeedSpanRows + threadIdx.x;
    unsigned long long sum = 0, w = 0;
    uint32_t row = kNoRow;
    if (i < (uint64_t)p.total_blocks * 32 && gld(&a.rinv[i]) != 0.0f) {
        const RowRef r = row_ref(p, (uint32_t)i);
        const float4* y[1] = {cx};
        double acc[1];
        pair_sums<1>(r.x, y, p.D4, acc, 32);
        const double c = finish_score(PCV_METRIC_COSINE, acc[0], gld(&a.norm[i]), nc);
        double cov = gld(&a.cover[i]);
        if (c > cov) {  // (both rows have a cosine: c is a number)
            cov = c;
            gst(&a.cover[i], cov);
        }
        w = seed_weight(cov);
        sum = w;
        if (w) row = (uint32_t)i;
    }
    seed_reduce(sh, sum, w, row);
    if (threadIdx.x == 0) seed_store_part(a, sum, w, row);
}

__global__ __launch_bounds__(kSeedSpanRows) void seed_pick_kernel(const ScanParams* __restrict__ pp, const SeedArgs a) {
    const ScanParams& p = *pp;
    __shared__ SeedShared sh;
    __shared__ uint32_t sel_span, sel_row;
    __shared__ unsigned long long sel_base;
    if (gld(&a.state->done)) return;
    if (threadIdx.x == 0) {  // (read behind the collectives below; a draw that no range holds would leave them: kSeedInternal)
        sel_span = 0;
        sel_base = 0;
        sel_row = kNoRow;
    }
    auto stop = [&](uint32_t error) {
        if (threadIdx.x == 0) {
            gst(&a.state->done, 1u);
            gst(&a.state->error, error);
        }
    };
    // each thread a run of consecutive partials: the threads' sums are in position order
    const uint32_t run = (a.parts + kSeedSpanRows - 1) / kSeedSpanRows;
    const uint32_t g0 = min(a.parts, threadIdx.x * run), g1 = min(a.parts, g0 + run);
    unsigned long long mine = 0, bw = 0;
    uint32_t br = kNoRow;
    for (uint32_t g = g0; g < g1; ++g) {
        const SeedPart* q = &a.part[g];
        mine += gld(&q->sum);
        const unsigned long long w = gld(&q->w);
        const uint32_t row = gld(&q->row);
        if (seed_before(w, row, bw, br)) {
            bw = w;
            br = row;
        }
    }
    unsigned long long T = mine;
    seed_reduce(sh, T, bw, br);
    if (T == 0) return stop(0);
    if (a.step == 0 && T > kMaxSeedRows) return stop(kSeedTooManyRows);
    uint32_t pick;
    if (a.step == 0 && a.has_first) {
        if (bw == 0) return stop(kSeedNoFirst);
        pick = br;
    } else if (a.method == PCV_SEED_FARTHEST) {
        pick = br;
    } else {
        const unsigned long long t = seed_draw(a.seed, (uint32_t)a.step, T);
        const unsigned long long incl = seed_scan(sh, mine);
        if (t >= incl - mine && t < incl) {  // (one thread: the ranges are disjoint and cover [0, T))
            unsigned long long base = incl - mine;
            uint32_t g = g0;
            for (; g + 1 < g1; ++g) {
                const unsigned long long s = gld(&a.part[g].sum);
                if (t < base + s) break;
                base += s;
            }
            sel_span = g;
            sel_base = base;
        }
        __syncthreads();
        const uint64_t i = (uint64_t)sel_span * kSeedSpanRows + threadIdx.x;
        unsigned long long w = 0;
        if (i < (uint64_t)p.total_blocks * 32 && gld(&a.rinv[i]) != 0.0f) w = a.step == 0 ? 1ull : seed_weight(gld(&a.cover[i]));
        const unsigned long long upto = sel_base + seed_scan(sh, w);
        if (t >= upto - w && t < upto) sel_row = (uint32_t)i;  // (one thread: the span's weights sum to its partial)
        __syncthreads();
        pick = sel_row;
    }
    if (pick == kNoRow) return stop(kSeedInternal);
    if (threadIdx.x == 0) {
        const RowRef r = row_ref(p, pick);
        gst(&a.out_ids[a.step], seed_id_of(r));
        gst(&a.out_pos[a.step], gld(&r.sg->pos0) + (int64_t)r.row);
        gst(&a.out_totals[a.step], (int64_t)T);
        gst(&a.out_cover[a.step], a.step == 0 ? __builtin_nanf("") : (float)gld(&a.cover[pick]));
        gst(&a.state->centre, pick);
        gst(&a.state->count, (int32_t)(a.step + 1));
    }
}

void check_seed_args(const ScanParams& p, const SeedArgs& a) {
    PCV_REQUIRE(p.total_blocks > 0 && a.parts == cdiv64((int64_t)p.total_blocks * 32, kSeedSpanRows) && a.step >= 0 && a.step < (int)PCV_MAX_SEEDS,
                "seeds: %u partials for %u blocks, step %d", a.parts, p.total_blocks, a.step);
}

}  // namespace

void launch_seed_begin(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SeedArgs& a) {
    check_seed_args(p, a);
    seed_begin_kernel<<<a.parts, kSeedSpanRows, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

void launch_seed_cover(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SeedArgs& a) {
    check_seed_args(p, a);
    seed_cover_kernel<<<a.parts, kSeedSpanRows, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

void launch_seed_pick(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SeedArgs& a) {
    check_seed_args(p, a);
    seed_pick_kernel<<<1, kSeedSpanRows, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

}  // namespace pcv
