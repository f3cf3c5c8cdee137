// moments_kernels.hip — the device steps of pcv_searcher_moments and pcv_searcher_project (DESIGN.md §4 "Corpus moments and principal
// axes"): the integer first and second moments of the fixed-point unit rows, and the canonical score of every row with m axes.
//
//   0. selfjoin_prep_kernel  (selfjoin_kernels.hip, unchanged) the canonical |x|^2 per launch row; rinv == 0: the row takes no part.
//   1. moment_sums_kernel    S_d = sum of t(r, d) in int64 and the number of participating rows (the arithmetic of label_sums_kernel:
//                            unit_int, launch_rows.h).
//   2. moment_syrk_kernel    C = T^T T by limbs (scan.h, MomentArgs): t = h * 2^16 + l, the limbs exact in f32, and
//                            HH = H^T H, HL = H^T L, LL = L^T L on v_mfma_f64_16x16x4_f64.  Every limb product is below 2^32.01 and a
//                            workgroup's chain is at most 2^20 rows long, so its f64 accumulators hold exact integers whatever order
//                            the hardware adds in; they are converted to int64 (exact) and added to the three matrices with 64-bit
//                            integer atomics, which are associative: the result is the same bits for any grid.
//   3. project_kernel        one thread per launch row: pair_sums (device_access.h) of the row with a group of axes read through
//                            wave-uniform pointers, then (float)(a * rinv - offset), the two steps rounded separately.
#include "device_access.h"
#include "launch_rows.h"
#include "row_jobs.h"

namespace pcv {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kSumBlocks = 8;     // row blocks of one moment_sums workgroup
constexpr int kMomentLdsRow = 80; // floats between two rows of a staged limb matrix: the four rows a wave reads in one instruction
                                  // start 80 banks apart, 16 lanes each

// grid: x = kSumBlocks row blocks; thread = one 16-byte piece of four features (pieces tid, tid + 256, ...)
__global__ __launch_bounds__(256) void moment_sums_kernel(const ScanParams* __restrict__ pp, const MomentArgs a) {
    const ScanParams& p = *pp;
    const int D4 = p.D4;
    const uint32_t gb0 = blockIdx.x * kSumBlocks, gb1 = min(p.total_blocks, gb0 + kSumBlocks);
    for (int f = threadIdx.x; f < D4; f += 256) {
        long long s0 = 0, s1 = 0, s2 = 0, s3 = 0, members = 0;
        int si = 0;
        for (uint32_t gb = gb0; gb < gb1; ++gb) {
            si = find_seg(p, gb, si);
            const SegDesc* sg = &p.seg[si];
            const float4* blk = gld(&sg->blk) + ((size_t)(gb - gld(&sg->blk0)) * D4 + f) * 32;
            for (int r = 0; r < 32; ++r) {
                const double n = gld(&a.norm[(size_t)gb * 32 + r]);
                if (!has_cosine(n)) continue;  // (the prep step leaves 0 for a row that takes no part)
                const double rs = unit_scale(n);
                const float4 v = gld4(blk + r);
                s0 += unit_int(v.x, rs);
                s1 += unit_int(v.y, rs);
                s2 += unit_int(v.z, rs);
                s3 += unit_int(v.w, rs);
                ++members;
            }
        }
        long long* d = a.sums + 4 * f;
        if (s0) g_atomic_add_i64(d, s0);
        if (s1) g_atomic_add_i64(d + 1, s1);
        if (s2) g_atomic_add_i64(d + 2, s2);
        if (s3) g_atomic_add_i64(d + 3, s3);
        if (f == 0 && members) g_atomic_add_i64(a.sums + 4 * D4, members);
    }
}

__device__ __forceinline__ void split_limbs(float x, double rs, float& h, float& l) {
    const long long t = rs != 0.0 ? unit_int(x, rs) : 0ll;  // (a row that takes no part may hold anything)
    h = (float)(t >> 16);
    l = (float)(t & 0xffff);
}

// grid: x = super-tile (I, J) of kMomentSide x kMomentSide outputs, all of them; y = row range.  Four waves; wave w owns the 16
// output rows (features of side I) 16 w .. 16 w + 15 and all four 16-column tiles of side J: HL always, HH and LL where J >= I.
// A block of 32 rows is staged as f32 limbs, [side][limb][row][feature]; per MFMA (four rows) lane (c = lane & 15, q = lane >> 4)
// holds A[feature c][row q] and B[row q][feature c], and in accumulator register i the output (row q + 4 i, column c).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void moment_syrk_kernel(const ScanParams* __restrict__ pp, const MomentArgs a) {
    const ScanParams& p = *pp;
    __shared__ float sh[2][2][32][kMomentLdsRow];
    const int D4 = p.D4, Dp = D4 * 4, tiles = Dp / kMomentSide;
    const int I = blockIdx.x / tiles, J = blockIdx.x % tiles;
    const bool upper = J >= I;
    const uint32_t b0 = blockIdx.y * a.range_blocks, b1 = min(p.total_blocks, b0 + a.range_blocks);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, kq = lane >> 4;
    const int r = threadIdx.x & 31, pc0 = threadIdx.x >> 5;  // the thread stages row r of pieces pc0, pc0 + 8 (side I), + 16, + 24 (side J)

    f64x4 HL[4], HH[4], LL[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) HL[j] = HH[j] = LL[j] = f64x4{0.0, 0.0, 0.0, 0.0};

    float4 v[4];
    double rs = 0.0;
    JoinSeg sc;  // (wave-uniform, in scalar registers: looked up again only where a segment ends)
    auto load = [&](uint32_t gb) {
        join_seek(p, sc, gb);
        const float4* blk = sc.blk + (size_t)(gb - sc.begin) * D4 * 32 + r;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = gld4(blk + (size_t)((q < 2 ? I : J) * 16 + ((pc0 + 8 * q) & 15)) * 32);
        const double n = gld(&a.norm[(size_t)gb * 32 + r]);
        rs = has_cosine(n) ? unit_scale(n) : 0.0;
    };
    if (b0 < b1) load(b0);
    for (uint32_t gb = b0; gb < b1; ++gb) {
        __syncthreads();  // (the block before this one has been read)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 h, l;
            split_limbs(v[q].x, rs, h.x, l.x);
            split_limbs(v[q].y, rs, h.y, l.y);
            split_limbs(v[q].z, rs, h.z, l.z);
            split_limbs(v[q].w, rs, h.w, l.w);
            const int f = 4 * ((pc0 + 8 * q) & 15);
            *reinterpret_cast<float4*>(&sh[q >> 1][0][r][f]) = h;
            *reinterpret_cast<float4*>(&sh[q >> 1][1][r][f]) = l;
        }
        __syncthreads();
        if (gb + 1 < b1) load(gb + 1);  // in flight under the MFMAs
#pragma unroll 2
        for (int s = 0; s < 8; ++s) {
            const int row = 4 * s + kq;
            const double ah = (double)sh[0][0][row][16 * wave + c], al = (double)sh[0][1][row][16 * wave + c];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double bh = (double)sh[1][0][row][16 * j + c], bl = (double)sh[1][1][row][16 * j + c];
                HL[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ah, bl, HL[j], 0, 0, 0);
                if (upper) {  // (the whole workgroup)
                    HH[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ah, bh, HH[j], 0, 0, 0);
                    LL[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(al, bl, LL[j], 0, 0, 0);
                }
            }
        }
    }
    // the end of the chain: exact integers below 2^53
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const size_t at = (size_t)(I * kMomentSide + 16 * wave + kq + 4 * i) * Dp + (size_t)(J * kMomentSide + 16 * j + c);
            const long long xhl = (long long)HL[j][i];
            if (xhl) g_atomic_add_i64(a.hl + at, xhl);
            if (upper) {
                const long long xhh = (long long)HH[j][i], xll = (long long)LL[j][i];
                if (xhh) g_atomic_add_i64(a.hh + at, xhh);
                if (xll) g_atomic_add_i64(a.ll + at, xll);
            }
        }
    }
}

// one thread per launch row; the axes in groups of NY: one pass over the row's pieces per group
template <int NY>
__global__ __launch_bounds__(256) void project_kernel(const ScanParams* __restrict__ pp, const ProjectArgs a) {
    const ScanParams& p = *pp;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)p.total_blocks * 32) return;
    const RowRef r = row_ref(p, (uint32_t)i);
    if (r.row >= gld(&r.sg->nrows)) return;
    const int64_t o = gld(&a.seg_out0[r.sg - p.seg]) + (int64_t)r.row;
    if (a.out_ids) {
        const int64_t* ids = gld(&r.sg->ids);
        gst(&a.out_ids[o], ids ? gld(&ids[r.row]) : gld(&r.sg->id0) + (int64_t)r.row);
    }
    float* out = a.out_coords + (size_t)o * a.m;
    if (gld(&a.rinv[i]) == 0.0f) {
        for (int j = 0; j < a.m; ++j) gst(&out[j], __builtin_nanf(""));
        return;
    }
    const double rinv = (double)(float)(1.0 / sqrt(gld(&a.norm[i])));  // (the f32 rinv of the prep step, also where that marks wild)
    for (int g = 0; g < a.m; g += NY) {  // (the packed axes are padded with zero axes up to a whole block)
        const float4* y[NY];
#pragma unroll
        for (int u = 0; u < NY; ++u) y[u] = uniform_ptr(a.axes + (size_t)((g + u) >> 5) * p.D4 * 32 + ((g + u) & 31));
        double acc[NY];
        pair_sums<NY>(r.x, y, p.D4, acc, 32);
#pragma unroll
        for (int u = 0; u < NY; ++u)
            if (g + u < a.m) gst(&out[g + u], (float)__dsub_rn(__dmul_rn(acc[u], rinv), gld(&a.offsets[g + u])));
    }
}

}  // namespace

void launch_moment_sums(hipStream_t st, const ScanParams& p, const ScanParams* dp, const MomentArgs& a) {
    if (p.total_blocks == 0) return;
    moment_sums_kernel<<<(p.total_blocks + kSumBlocks - 1) / kSumBlocks, 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

uint32_t moment_row_ranges(const ScanParams& p, const MomentArgs& a) { return (p.total_blocks + a.range_blocks - 1) / a.range_blocks; }

void launch_moment_syrk(hipStream_t st, const ScanParams& p, const ScanParams* dp, const MomentArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t tiles = (uint32_t)(p.D4 * 4 / kMomentSide), ranges = a.range_blocks ? moment_row_ranges(p, a) : 0;
    PCV_REQUIRE(p.D4 % 16 == 0 && a.range_blocks >= 1 && a.range_blocks <= kMomentChainBlocks && ranges <= 65535u,
                "moments: bad launch (%d pieces, %u blocks a chain, %u ranges)", p.D4, a.range_blocks, ranges);
    moment_syrk_kernel<<<dim3(tiles * tiles, ranges), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

void launch_project(hipStream_t st, const ScanParams& p, const ScanParams* dp, const ProjectArgs& a) {
    if (p.total_blocks == 0) return;
    PCV_REQUIRE(a.m >= 1 && a.m <= (int)PCV_MAX_AXES, "project: %d axes", a.m);
    const unsigned grid = cdiv64((int64_t)p.total_blocks * 32, 256);
    if (a.m <= 2)
        project_kernel<2><<<grid, 256, 0, st>>>(dp, a);
    else
        project_kernel<8><<<grid, 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

}  // namespace pcv
