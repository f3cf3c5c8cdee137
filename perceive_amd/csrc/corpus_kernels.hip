// corpus_kernels.hip — gfx950 kernels that build and maintain a corpus segment: staging rows into the blocked layout, row
// scales, the screening copies (bf16, int8, 6-bit) and the mid copy (scan.h), and what changes a finalized segment in place —
// hiding, unhiding, updating and removing items by id, views, search by example.  None of the search-path kernels
// (scan_kernels.hip) is involved; the launchers are declared in corpus.h.
//
// A repacked row or block must get exactly the bits a fresh build gives it (hide / unhide, update and remove rest on that), so
// every piece of row arithmetic that both a build kernel and a repack kernel need exists once, in the helpers below.
#include <algorithm>
#include <cassert>

#include "common.h"
#include "corpus.h"
#include "device_access.h"
#include "scan.h"
#include "synth.h"

namespace pcv {
namespace {

// ------------------------------------------------------------------------------------------------
// row arithmetic shared by the build kernels and the repack kernels
// ------------------------------------------------------------------------------------------------

// Piece f4 of a staged row-major f32 row of D features, as the blocked layout stores it: zeros past D.
__device__ __forceinline__ float4 staged_piece(const float* __restrict__ row, int f4, int D) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f = f4 * 4 + j;
        v[j] = f < D ? row[f] : 0.0f;
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

// |x|^2 of a row of D4 pieces, accumulated in f64 in feature order; piece(f4) gives the row's float4 number f4 (from the
// blocked layout, from a staged row, from the generator: the same values give the same sum).
template <class Piece>
__device__ __forceinline__ double row_sum_squares(int D4, Piece piece) {
    double nx = 0.0;
    for (int f4 = 0; f4 < D4; ++f4) {
        const float4 v = piece(f4);
        nx += (double)v.x * (double)v.x;
        nx += (double)v.y * (double)v.y;
        nx += (double)v.z * (double)v.z;
        nx += (double)v.w * (double)v.w;
    }
    return nx;
}
__device__ __forceinline__ double blocked_row_sum_squares(const float4* __restrict__ blk, uint32_t row, int D4) {
    const float4* base = blk + (size_t)(row >> 5) * D4 * 32 + (row & 31);
    return row_sum_squares(D4, [&](int f4) { return base[(size_t)f4 * 32]; });
}

// per-row scale = 1/|x| (cosine) or 1 (dot) from nx = |x|^2; 0 marks rows that can never be a result (zero / non-finite norm)
__device__ __forceinline__ float row_scale(double nx, int metric) {
    const bool finite = nx < __builtin_inf();  // false for inf and NaN
    if (metric == PCV_METRIC_DOT) return finite ? 1.0f : 0.0f;
    return (finite && nx >= 0x1p-126) ? (float)(1.0 / sqrt(nx)) : 0.0f;
}
// the corpus bound max_norm (an upper bound of |x|, dot metric margins) covers a row that has a scale; it only grows
__device__ __forceinline__ void raise_max_norm(uint32_t* max_norm_bits, double nx, float scale) {
    if (scale != 0.0f) {
        float nrm = (float)sqrt(nx) * 1.000001f;
        atomicMax(max_norm_bits, __builtin_bit_cast(uint32_t, nrm));
    }
}

// bf16 screening copy: piece f8 of row r of block b = bf16(RNE) of features 8*f8..8*f8+7 times the row's scale sc; rows that
// are not searchable (scale 0: padding, bad norm, hidden) become exact zeros.
__device__ __forceinline__ uint4 bf16_piece(const float4* __restrict__ blk, float sc, uint32_t b, uint32_t f8, uint32_t r, int D4) {
    uint4 out = make_uint4(0, 0, 0, 0);
    if (sc != 0.0f) {
        const float4 lo = blk[((size_t)b * D4 + 2 * f8) * 32 + r], hi = blk[((size_t)b * D4 + 2 * f8 + 1) * 32 + r];
        const f32x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        out = __builtin_bit_cast(uint4, __builtin_convertvector(v * sc, bf16x8));  // the conversion the f32 scan kernel does
    }
    return out;
}

// The largest quantisation scale a copy is given.  127 / max (int8) and 32766 / max (mid) are inf once the largest feature of a
// dot-metric block or row is below 127 / FLT_MAX = 3.73e-37 (9.6e-35 for the mid scale) — still normal f32 values.  Any scale s at
// or below 127 / max (32766 / max) keeps the codes inside their range and |y_i - code_i / s| <= 0.5 / s, which is all the bounds of
// scan.h use — the tests are the same inequalities with this s — so the scale is capped: such a block gets all-zero codes and
// |y_i| <= 0.5 / s = 2^-101 is true of it.  Under the cosine max|y_i| >= 1 / sqrt(dim): the cap is never reached.
constexpr float kMaxCopyScale = 0x1p100f;

// Int8 screening copy of block b by one wave: lane (r, h) owns row r and every other 16-feature piece.  Pass 1: max |y_i| over
// the BLOCK's searchable rows (y = x * scale); pass 2: x^_i = rint(y_i * s_blk),
// s_blk = 127 / max: one scale for the 32 rows, so the scan's test of a block needs one float and its right-hand side is the same
// for every row (per row scales made the block pre-test loose — the smallest scale of 16 rows stood for all of them, a third
// of the blocks of a 12.5M-row pass went on to the row-by-row test at ~2 us each — and cost 144 B per block).  A row
// quantised with a smaller scale than its own 127 / max|y_i| keeps |x^_i| <= 127 and |y_i - x^_i / s| <= 0.5 / s: the bound of
// scan.h holds with s = s_blk; on Gaussian rows the margin grows by ~7 %.  Rows that are not searchable are stored as zeros (they
// reach the fine screen only under a non-positive right-hand side and end there: scale 0); a block without a searchable row
// gets s_blk = NaN (no comparison succeeds); all-zero searchable rows (dot metric) alone: s_blk = 1.
__device__ __forceinline__ void pack8_block(const float4* __restrict__ blk, const float* __restrict__ scale, uint4* __restrict__ blk8,
                                            float* __restrict__ scale8, uint32_t b, int D4, int D16, int lane) {
    const int r = lane & 31, h = lane >> 5;
    const float sc = scale[(size_t)b * 32 + r];
    const float4* src = blk + (size_t)b * D4 * 32 + r;
    float mx = 0.0f;
    for (int g = h; g < D16; g += 2)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * g + e < D4) {
                const float4 v = src[(size_t)(4 * g + e) * 32];
                mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v.x * sc), fabsf(v.y * sc)), fmaxf(fabsf(v.z * sc), fabsf(v.w * sc))));
            }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const bool searchable = sc != 0.0f && mx < __builtin_inff();  // (NaN features: fmaxf ignores them; such rows have scale 0)
    float bm = searchable ? mx : 0.0f;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) bm = fmaxf(bm, __shfl_xor(bm, off));
    const bool any_row = __any(searchable);
    const float s_blk = !any_row ? __builtin_nanf("") : (bm > 0.0f ? fminf(127.0f / bm, kMaxCopyScale) : 1.0f);
    for (int g = h; g < D16; g += 2) {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (searchable && 4 * g + e < D4) {
                const float4 v = src[(size_t)(4 * g + e) * 32];
                const float y[4] = {v.x * sc, v.y * sc, v.z * sc, v.w * sc};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int qv = max(-127, min(127, (int)rintf(y[j] * s_blk)));
                    w[e] |= (uint32_t)(qv & 0xff) << (8 * j);
                }
            }
        blk8[((size_t)b * D16 + g) * 32 + r] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (lane == 0) scale8[b] = s_blk;
}

// Mid copy (scan.h): two features y0, y1 = x * scale of a row -> their int16 codes rint(y * s2), clamped, in one word; a row
// that is not searchable is stored as zeros, with a NaN scale.
__device__ __forceinline__ uint32_t mid_pair(float y0, float y1, float s2, bool searchable) {
    const int lo = searchable ? max(-32767, min(32767, (int)rintf(y0 * s2))) : 0;
    const int hi = searchable ? max(-32767, min(32767, (int)rintf(y1 * s2))) : 0;
    return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
}
// the mid scale of the rows of a block whose int8 copy has the scale s_blk (the int8 copy's block maximum: any
// s2 <= 32766 / max|y_i| of a row keeps |y_i - Y_i / s2| <= 0.5 / s2, which is all the mid screen's bound uses); NaN: a block
// without a searchable row
__device__ __forceinline__ float mid_block_scale(float s_blk) { return s_blk * (32766.0f / 127.0f); }
__device__ __forceinline__ float mid_stored_scale(float s2, bool searchable) { return searchable ? s2 : __builtin_nanf(""); }

// Mid copy of one row by one wave: lane j < Dp/8 owns the 8 features 8j..8j+7 (two pieces of the blocked row), the 16 bytes go
// out as part of the row's Dp * 2 contiguous ones.  scale8 == nullptr: the row's own s2 = 32766 / max|y_i| (the maximum goes
// round the wave); otherwise the scale of the row's block, mid_block_scale(scale8[b]).
__device__ __forceinline__ void mid_pack_row(const float4* __restrict__ blk, const float* __restrict__ scale,
                                             const float* __restrict__ scale8, uint4* __restrict__ mid16, float* __restrict__ scale16,
                                             uint32_t row, int D4, int lane) {
    const int P8 = D4 >> 1;  // 16-byte pieces of a mid row
    const float sc = scale[row];
    const float4* src = blk + (size_t)(row >> 5) * D4 * 32 + (row & 31);
    float s2;
    bool searchable;
    if (scale8) {
        s2 = mid_block_scale(scale8[row >> 5]);
        searchable = sc != 0.0f && s2 == s2;
    } else {
        float mx = 0.0f;
        for (int j = lane; j < P8; j += 64) {
            const float4 a = src[(size_t)(2 * j) * 32], b = src[(size_t)(2 * j + 1) * 32];
            mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(fabsf(a.x * sc), fabsf(a.y * sc)), fmaxf(fabsf(a.z * sc), fabsf(a.w * sc))),
                                 fmaxf(fmaxf(fabsf(b.x * sc), fabsf(b.y * sc)), fmaxf(fabsf(b.z * sc), fabsf(b.w * sc)))));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        searchable = sc != 0.0f && mx < __builtin_inff();
        s2 = !searchable ? 0.0f : (mx > 0.0f ? fminf(32766.0f / mx, kMaxCopyScale) : 1.0f);
    }
    for (int j = lane; j < P8; j += 64) {
        const float4 a = src[(size_t)(2 * j) * 32], b = src[(size_t)(2 * j + 1) * 32];
        mid16[(size_t)row * P8 + j] = make_uint4(mid_pair(a.x * sc, a.y * sc, s2, searchable), mid_pair(a.z * sc, a.w * sc, s2, searchable),
                                                 mid_pair(b.x * sc, b.y * sc, s2, searchable), mid_pair(b.z * sc, b.w * sc, s2, searchable));
    }
    if (lane == 0) scale16[row] = mid_stored_scale(s2, searchable);
}

// A batch of ids is looked up in an open-addressed table (corpus.h: id_hash, linear probing, kIdEmpty in free slots; a batch that
// holds kIdEmpty itself says so with has_empty).  `slot`: where in the table the id was found; kNoSlot for kIdEmpty, which has none.
constexpr uint32_t kNoSlot = 0xffffffffu;
struct IdProbe {
    bool hit;
    uint32_t slot;
};
__device__ __forceinline__ IdProbe probe_id(int64_t id, const int64_t* __restrict__ table, uint32_t tmask, int has_empty) {
    if (id == kIdEmpty) return {has_empty != 0, kNoSlot};
    for (uint32_t h = id_hash(id, tmask);; h = (h + 1) & tmask) {
        const int64_t t = table[h];
        if (t == id) return {true, h};
        if (t == kIdEmpty) return {false, kNoSlot};
    }
}

// ------------------------------------------------------------------------------------------------
// ingestion-time kernels
// ------------------------------------------------------------------------------------------------

// row-major staging [n][D] -> blocked layout, rows row0.. of the segment (buffer pre-zeroed)
__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ rows, int64_t n, int D, int D4,
                                                        float4* __restrict__ blk, uint32_t row0) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(t & 31);
    const int64_t u = t >> 5;
    const int f4 = (int)(u % D4);
    const int64_t lb = u / D4;  // block relative to the first touched block
    const uint32_t first_blk = row0 >> 5;
    const int64_t row = (lb + first_blk) * 32 + r;  // row inside the segment
    const int64_t src = row - row0;
    if (src < 0 || src >= n) return;
    blk[((lb + first_blk) * D4 + f4) * 32 + r] = staged_piece(rows + src * D, f4, D);
}

__global__ __launch_bounds__(256) void iota_ids_kernel(int64_t* __restrict__ ids, int64_t first, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) ids[i] = first + i;
}

// scale of rows [row_begin, row_end) (row_scale above); rows >= nrows are padding: scale 0
__global__ __launch_bounds__(256) void row_scales_kernel(const float4* __restrict__ blk, uint32_t row_begin,
                                                         uint32_t row_end, uint32_t nrows, int D4, int metric,
                                                         float* __restrict__ scale, uint32_t* max_norm_bits) {
    const uint32_t row = row_begin + blockIdx.x * 256 + threadIdx.x;
    if (row >= row_end) return;
    float out = 0.0f;
    if (row < nrows) {
        const double nx = blocked_row_sum_squares(blk, row, D4);
        out = row_scale(nx, metric);
        raise_max_norm(max_norm_bits, nx, out);
    }
    scale[row] = out;
}

// bf16 screening copy (bf16_piece) of blocks [first_block, nblocks), one thread per piece
__global__ __launch_bounds__(256) void coarse_pack_kernel(const float4* __restrict__ blk, const float* __restrict__ scale,
                                                          uint4* __restrict__ blk16, uint32_t first_block, uint32_t nblocks, int D4) {
    const int D8 = D4 >> 1;
    const size_t per_block = (size_t)D8 * 32;
    const size_t total = (size_t)(nblocks - first_block) * per_block;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const uint32_t b = first_block + (uint32_t)(i / per_block);
        const uint32_t rem = (uint32_t)(i % per_block);
        const uint32_t f8 = rem >> 5, r = rem & 31;
        blk16[((size_t)b * D8 + f8) * 32 + r] = bf16_piece(blk, scale[(size_t)b * 32 + r], b, f8, r, D4);
    }
}

// Int8 screening copy (pack8_block) of blocks [first_block, nblocks), one wave per block
__global__ __launch_bounds__(256) void coarse_pack8_kernel(const float4* __restrict__ blk, const float* __restrict__ scale,
                                                           uint4* __restrict__ blk8, float* __restrict__ scale8, uint32_t first_block,
                                                           uint32_t nblocks, int D4) {
    const int lane = threadIdx.x & 63;
    const int D16 = ((D4 * 4 + 127) & ~127) >> 4;
    for (uint32_t b = first_block + blockIdx.x * 4 + (threadIdx.x >> 6); b < nblocks; b += gridDim.x * 4)
        pack8_block(blk, scale, blk8, scale8, b, D4, D16, lane);
}

// 6-bit copy (scan.h) of blocks [first_block, nblocks) — or of blocks[0..n) when `blocks` is given — from the int8 copy: one wave per
// block, lane (r, h) of the int8 layout packs the 64 codes it feeds the MFMAs of each chunk, u = (x^ >> 2) + 32, into its three
// pieces.  r_blk and n_blk are measured against the f32 rows (f64 sums, maxima over the block's searchable rows, rounded up), so the
// bound holds whatever the int8 copy's own rounding was.  Rows that are not searchable are left out of both (their int8 codes are
// zeros; they end at the fine screen: scale 0).
__global__ __launch_bounds__(256) void pack6_kernel(const float4* __restrict__ blk, const float* __restrict__ scale,
                                                    const uint4* __restrict__ blk8, const float* __restrict__ scale8,
                                                    const uint32_t* __restrict__ blocks, uint4* __restrict__ blk6,
                                                    float4* __restrict__ scale6, uint32_t first_block, uint32_t nblocks, int D4) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int D16 = ((D4 * 4 + 127) & ~127) >> 4, NCH = D16 >> 3;
    for (uint32_t i = (blocks ? 0u : first_block) + blockIdx.x * 4 + (threadIdx.x >> 6); i < nblocks; i += gridDim.x * 4) {
        const uint32_t b = blocks ? blocks[i] : i;
        const float sc = scale[(size_t)b * 32 + r];
        const float s = scale8[b];
        const bool searchable = sc != 0.0f && s == s;
        const double inv_s = searchable ? 1.0 / (double)s : 0.0;
        double e2 = 0.0, n2 = 0.0;
        for (int ch = 0; ch < NCH; ++ch) {
            uint32_t w[16];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int f16 = ch * 8 + 2 * ks + h;
                const uint4 v = blk8[((size_t)b * D16 + f16) * 32 + r];
                w[4 * ks] = v.x;
                w[4 * ks + 1] = v.y;
                w[4 * ks + 2] = v.z;
                w[4 * ks + 3] = v.w;
#pragma unroll
                for (int e = 0; e < 4; ++e) {  // the 16 features of the piece against the f32 row
                    const int f4 = 4 * f16 + e;
                    if (!searchable || f4 >= D4) continue;
                    const float4 x = blk[((size_t)b * D4 + f4) * 32 + r];
                    const float y[4] = {x.x * sc, x.y * sc, x.z * sc, x.w * sc};
                    const uint32_t word = w[4 * ks + e];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x8 = (int)(int8_t)(word >> (8 * j));
                        const double xt = (double)(4 * (x8 >> 2)) * inv_s + 1.5 * inv_s;
                        const double d = (double)y[j] - xt;
                        e2 += d * d;
                        n2 += xt * xt;
                    }
                }
            }
            uint32_t u[16];
#pragma unroll
            for (int d = 0; d < 16; ++d) {  // per byte: (x^ >> 2) + 32, i.e. the top six bits of x^ + 128
                const uint32_t biased = w[d] ^ 0x80808080u;  // x^ + 128 in each byte (no carries: x^ in [-127, 127])
                u[d] = (biased >> 2) & 0x3f3f3f3fu;
            }
            uint32_t lo[8], hi[4];
#pragma unroll
            for (int k = 0; k < 8; ++k) lo[k] = (u[2 * k] & 0x0f0f0f0fu) | ((u[2 * k + 1] & 0x0f0f0f0fu) << 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                hi[k] = 0;
#pragma unroll
                for (int m = 0; m < 4; ++m) hi[k] |= ((u[4 * k + m] >> 4) & 0x03030303u) << (2 * m);
            }
            uint4* dst = blk6 + ((size_t)b * NCH + ch) * 3 * 64 + lane;
            dst[0] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
            dst[64] = make_uint4(lo[4], lo[5], lo[6], lo[7]);
            dst[128] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        }
        e2 += __shfl_xor(e2, 32);
        n2 += __shfl_xor(n2, 32);
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) {
            e2 = fmax(e2, __shfl_xor(e2, off));
            n2 = fmax(n2, __shfl_xor(n2, off));
        }
        if (lane == 0) {
            const float up = 1.0f + 0x1p-19f;
            const bool any = s == s;
            scale6[b] = make_float4(s, any ? (float)(sqrt(e2) * (double)s) * up : 0.0f, any ? (float)(sqrt(n2) * (double)s) * up : 0.0f, 0.0f);
        }
    }
}

// Mid copy (mid_pack_row, each row with its own scale) of rows [first_row, nrows), one wave per row at a time
__global__ __launch_bounds__(256) void mid_pack_kernel(const float4* __restrict__ blk, const float* __restrict__ scale, uint4* __restrict__ mid16,
                                                       float* __restrict__ scale16, uint32_t first_row, uint32_t nrows, int D4) {
    const int lane = threadIdx.x & 63;
    for (uint32_t row = first_row + blockIdx.x * 4 + (threadIdx.x >> 6); row < nrows; row += gridDim.x * 4)
        mid_pack_row(blk, scale, nullptr, mid16, scale16, row, D4, lane);
}

// The same copy for segments that have their int8 screening copy (the normal case), one wave per 32-row BLOCK: the block's
// pieces are read as the scan reads them — two contiguous 512-byte runs per instruction, every row once — quantised with ONE
// scale for the block, mid_block_scale(scale8[b]) (no pass for the maximum), turned row-major in LDS
// and written as the block's Dp * 64 contiguous bytes.  mid_pack_kernel above gathers 16-byte pieces 512 bytes apart, twice per
// row: 1.0 TB/s, 228 ms per 100M x 384 rows (profiles/r03_batch256_kernel_stats.csv).
__global__ __launch_bounds__(64) void mid_pack_block_kernel(const float4* __restrict__ blk, const float* __restrict__ scale,
                                                            const float* __restrict__ scale8, uint4* __restrict__ mid16,
                                                            float* __restrict__ scale16, uint32_t first_block, uint32_t nblocks, int D4) {
    extern __shared__ uint2 mtile[];  // [32][D4 + 2]: a row's 8-byte pieces, two of padding (rows stay 16-byte aligned)
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int LD = D4 + 2, P2 = D4 >> 1;
    for (uint32_t b = first_block + blockIdx.x; b < nblocks; b += gridDim.x) {
        const float sc = scale[(size_t)b * 32 + r];
        const float s2 = mid_block_scale(scale8[b]);
        const bool searchable = sc != 0.0f && s2 == s2;
        const float4* src = blk + (size_t)b * D4 * 32 + h * 32 + r;  // piece 2j + h of row r: src + 64 j
        for (int j0 = 0; j0 < P2; j0 += 16) {  // 16 KB of a block requested at a time (six waves a CU at 384-d: ~100 KB in flight)
            float4 v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (j0 + u < P2) v[u] = ld_row<true>(src + (size_t)(j0 + u) * 64);
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (j0 + u < P2) {
                    mtile[r * LD + 2 * (j0 + u) + h] = make_uint2(mid_pair(v[u].x * sc, v[u].y * sc, s2, searchable),
                                                                  mid_pair(v[u].z * sc, v[u].w * sc, s2, searchable));
                }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the tile is written (one wave: nobody else touches it)
        __builtin_amdgcn_wave_barrier();
        uint4* dst = mid16 + (size_t)b * 32 * P2;
        for (int i = lane; i < 32 * P2; i += 64) {
            const int row = i / P2, pc = i - row * P2;
            dst[i] = *(const uint4*)&mtile[row * LD + 2 * pc];
        }
        if (lane < 32) scale16[(size_t)b * 32 + lane] = mid_stored_scale(s2, searchable);
        __builtin_amdgcn_s_waitcnt(0xc07f);  // the reads are done before the next block overwrites the tile
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------------
// hidden items (pcv_searcher_hide_ids, DESIGN.md §3 "Hidden items"): rows found by id and switched to "not searchable"
// (scale 0, zeros in the screening copies, NaN mid scale) in place, or back.  None of the kernels above is involved.
// ------------------------------------------------------------------------------------------------

// Rows [row0, row1) of a segment whose id is in the batch's hash table (probe_id): their in-segment row numbers are
// appended to out_rows (the first `cap` of them; *out_n counts all).  One id per lane, one atomic per wave.
__global__ __launch_bounds__(256) void match_ids_kernel(const int64_t* __restrict__ ids, uint32_t row0, uint32_t row1,
                                                        const int64_t* __restrict__ table, uint32_t tmask, int has_empty,
                                                        uint32_t* __restrict__ out_rows, uint32_t* __restrict__ out_n, uint32_t cap) {
    const int lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)row0 + (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < row1;
         base += (uint64_t)gridDim.x * 256) {
        const uint32_t row = (uint32_t)base + lane;
        const bool hit = row < row1 && probe_id(__builtin_nontemporal_load(&ids[row]), table, tmask, has_empty).hit;
        const unsigned long long ball = __ballot(hit);
        if (ball) {
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(out_n, (uint32_t)__popcll(ball));
            at = __shfl(at, 0);
            if (hit) {
                const uint32_t i = at + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
                if (i < cap) out_rows[i] = row;
            }
        }
    }
}

// Hide rows[0..n) of a segment, one wave per row: scale 0, its int8 / bf16 pieces zero (rows < copied_rows), its mid scale NaN
// (rows < mid_rows).  The int8 block scale stays: fewer searchable rows under the same s_blk keep the bound of scan.h.
__global__ __launch_bounds__(256) void hide_rows_kernel(const uint32_t* __restrict__ rows, uint32_t n, float* __restrict__ scale,
                                                        uint4* __restrict__ blk8, uint4* __restrict__ blk16, uint32_t copied_rows,
                                                        float* __restrict__ scale16, uint32_t mid_rows, int D4) {
    const int lane = threadIdx.x & 63;
    const int D8 = D4 >> 1, D16 = ((D4 * 4 + 127) & ~127) >> 4;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        const uint32_t row = rows[i], b = row >> 5, r = row & 31;
        if (lane == 0) {
            scale[row] = 0.0f;
            if (scale16 && row < mid_rows) scale16[row] = __builtin_nanf("");
        }
        if (row < copied_rows) {
            if (blk8)
                for (int g = lane; g < D16; g += 64) blk8[((size_t)b * D16 + g) * 32 + r] = make_uint4(0, 0, 0, 0);
            if (blk16)
                for (int f8 = lane; f8 < D8; f8 += 64) blk16[((size_t)b * D8 + f8) * 32 + r] = make_uint4(0, 0, 0, 0);
        }
    }
}

// Unhide, step 1: the scale of rows[0..n), one thread per row, as row_scales_kernel gives it.  The corpus bound max_norm only
// grows: it already covers these rows.
__global__ __launch_bounds__(256) void restore_scales_kernel(const float4* __restrict__ blk, const uint32_t* __restrict__ rows,
                                                             uint32_t n, int D4, int metric, float* __restrict__ scale) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = rows[i];
    scale[row] = row_scale(blocked_row_sum_squares(blk, row, D4), metric);
}

// Unhide, step 2 (int8 copy): blocks[0..n) re-packed whole (pack8_block): s_blk is taken
// again over the block's searchable rows, the returned ones among them (a finalize that appended rows to the block while they
// were hidden set it without them: it may exceed 127 / max|y_i| of a returned row, whose values would then clip).
__global__ __launch_bounds__(256) void repack8_blocks_kernel(const float4* __restrict__ blk, const float* __restrict__ scale,
                                                             const uint32_t* __restrict__ blocks, uint32_t n, uint4* __restrict__ blk8,
                                                             float* __restrict__ scale8, int D4) {
    const int lane = threadIdx.x & 63;
    const int D16 = ((D4 * 4 + 127) & ~127) >> 4;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4)
        pack8_block(blk, scale, blk8, scale8, blocks[i], D4, D16, lane);
}

// Unhide, step 2 (bf16 copy): the pieces (bf16_piece) of rows[0..n), one wave per row (the piece is row-local).
__global__ __launch_bounds__(256) void repack16_rows_kernel(const float4* __restrict__ blk, const float* __restrict__ scale,
                                                            const uint32_t* __restrict__ rows, uint32_t n, uint4* __restrict__ blk16, int D4) {
    const int lane = threadIdx.x & 63;
    const int D8 = D4 >> 1;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        const uint32_t row = rows[i], b = row >> 5, r = row & 31;
        const float sc = scale[row];
        for (int f8 = lane; f8 < D8; f8 += 64) blk16[((size_t)b * D8 + f8) * 32 + r] = bf16_piece(blk, sc, b, f8, r, D4);
    }
}

// Unhide, step 3 (mid copy), one wave per row (mid_pack_row), rows < mid_rows only.  scale8 != nullptr (the segment has its int8
// copy): items[] are blocks and every row of each is re-quantised with the scale of the re-packed block, as mid_pack_block_kernel
// does; otherwise items[] are rows, each with its own scale, as mid_pack_kernel does.
__global__ __launch_bounds__(256) void repack_mid_kernel(const float4* __restrict__ blk, const float* __restrict__ scale,
                                                         const float* __restrict__ scale8, const uint32_t* __restrict__ items, uint32_t n,
                                                         uint32_t mid_rows, uint4* __restrict__ mid16, float* __restrict__ scale16, int D4) {
    const int lane = threadIdx.x & 63;
    const uint32_t per = scale8 ? 32u : 1u;
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < (uint64_t)n * per; t += (uint64_t)gridDim.x * 4) {
        const uint32_t row = scale8 ? items[t >> 5] * 32 + (uint32_t)(t & 31) : items[t];
        if (row >= mid_rows) continue;
        mid_pack_row(blk, scale, scale8, mid16, scale16, row, D4, lane);
    }
}

// ------------------------------------------------------------------------------------------------
// updated items (pcv_searcher_update_rows, DESIGN.md §3 "Updated items"): new vectors written in place at the rows found by id;
// the screening and mid copies are then re-packed by the unhide kernels above.  None of the scan kernels is involved.
// ------------------------------------------------------------------------------------------------

// match_ids_kernel with the batch index: the table carries, next to each id, its slot in the batch (vals[h] for table[h]; the
// id kIdEmpty, if in the batch, has empty_slot).  Rows [row0, row1) of a segment whose id is in the batch -> (out_rows[i],
// out_slots[i]) for the first `cap` of them; *out_n counts all.  One id per lane, one atomic per wave.
__global__ __launch_bounds__(256) void match_id_slots_kernel(const int64_t* __restrict__ ids, uint32_t row0, uint32_t row1,
                                                             const int64_t* __restrict__ table, const uint32_t* __restrict__ vals,
                                                             uint32_t tmask, int has_empty, uint32_t empty_slot,
                                                             uint32_t* __restrict__ out_rows, uint32_t* __restrict__ out_slots,
                                                             uint32_t* __restrict__ out_n, uint32_t cap) {
    const int lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)row0 + (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < row1;
         base += (uint64_t)gridDim.x * 256) {
        const uint32_t row = (uint32_t)base + lane;
        bool hit = false;
        uint32_t slot = 0;
        if (row < row1) {
            const IdProbe pr = probe_id(__builtin_nontemporal_load(&ids[row]), table, tmask, has_empty);
            hit = pr.hit;
            if (hit) slot = pr.slot == kNoSlot ? empty_slot : vals[pr.slot];
        }
        const unsigned long long ball = __ballot(hit);
        if (ball) {
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(out_n, (uint32_t)__popcll(ball));
            at = __shfl(at, 0);
            if (hit) {
                const uint32_t i = at + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
                if (i < cap) {
                    out_rows[i] = row;
                    out_slots[i] = slot;
                }
            }
        }
    }
}

// Write the new vectors, one wave per (rows[i], slots[i]) pair: staged row slots[i] - slot0 (row-major [.][D] f32; bit 31 of
// slots[i] marks an id in the hidden set) goes into the blocked layout as pack_rows_kernel stores it.  Lane 0 then gives the row
// its scale as row_scales_kernel does (the same values, read from the staged row), raises max_norm as it does — hidden rows too,
// since unhiding relies on max_norm covering them — and stores scale 0 for a hidden row.
__global__ __launch_bounds__(256) void update_rows_kernel(const float* __restrict__ stage, uint32_t slot0,
                                                          const uint32_t* __restrict__ rows, const uint32_t* __restrict__ slots,
                                                          uint32_t n, int D, int D4, int metric, float4* __restrict__ blk,
                                                          float* __restrict__ scale, uint32_t* max_norm_bits) {
    const int lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        const uint32_t row = rows[i], sl = slots[i];
        const bool hidden = (sl >> 31) != 0;
        const float* src = stage + (size_t)((sl & 0x7fffffffu) - slot0) * D;
        float4* dst = blk + (size_t)(row >> 5) * D4 * 32 + (row & 31);
        for (int f4 = lane; f4 < D4; f4 += 64) dst[(size_t)f4 * 32] = staged_piece(src, f4, D);
        if (lane == 0) {
            const double nx = row_sum_squares(D4, [&](int f4) { return staged_piece(src, f4, D); });
            const float out = row_scale(nx, metric);
            raise_max_norm(max_norm_bits, nx, out);
            scale[row] = hidden ? 0.0f : out;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// views (pcv_searcher_create_view, DESIGN.md §3 "Views"): the rows of a parent segment whose id is in an allow list, copied in
// parent row order into the view's own blocked layout.  Selection keeps row order: a flag per row and a count per tile of
// kViewTile rows (view_mark_kernel), an exclusive scan of the tile counts (view_scan_kernel), then each tile writes its rows at
// its offset (view_compact_kernel).  None of the kernels above is involved.
// ------------------------------------------------------------------------------------------------
// (kViewTile, corpus.h: rows per tile — 4 consecutive rows per thread of a 256-thread workgroup)

// Exclusive prefix of one value per thread over a 256-thread workgroup; *total = the sum.  `part`: 4 words of LDS.
__device__ __forceinline__ uint32_t view_block_scan(uint32_t v, uint32_t* part, uint32_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) part[w] = x;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t p = part[i];
        base += i < w ? p : 0u;
        total += p;
    }
    __syncthreads();  // (part may be written again)
    return base + x - v;
}

// Rows of a segment whose id is in the batch's hash table (probe_id): flags4[tile * 256 + t] holds the flags of rows
// tile * kViewTile + 4t .. 4t + 3 in bits 0, 8, 16, 24; tile_cnt[tile] = how many rows of the tile are flagged.  `invert`: the
// rows whose id is NOT in the table are flagged (pcv_searcher_remove_ids: flag = the row stays); rows >= nrows are never flagged.
__global__ __launch_bounds__(256) void view_mark_kernel(const int64_t* __restrict__ ids, uint32_t nrows, const int64_t* __restrict__ table,
                                                        uint32_t tmask, int has_empty, int invert, uint32_t* __restrict__ flags4,
                                                        uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t part[4];
    const uint64_t r0 = (uint64_t)blockIdx.x * kViewTile + threadIdx.x * 4u;
    uint32_t f = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t row = r0 + j;
        if (row >= nrows) break;
        const bool hit = probe_id(__builtin_nontemporal_load(&ids[row]), table, tmask, has_empty).hit;
        if (hit != (invert != 0)) f |= 1u << (8 * j);
    }
    flags4[(size_t)blockIdx.x * 256 + threadIdx.x] = f;
    uint32_t total = 0;
    (void)view_block_scan((uint32_t)__popc(f), part, total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// tile_cnt[0..ntiles) -> their exclusive prefix sums in place, the sum -> *total.  One workgroup, each thread a contiguous run.
__global__ __launch_bounds__(256) void view_scan_kernel(uint32_t* __restrict__ tile_cnt, uint32_t ntiles, uint32_t* __restrict__ total) {
    __shared__ uint32_t part[4];
    const uint32_t per = (ntiles + 255) / 256;
    const uint32_t t0 = (uint32_t)std::min<uint64_t>((uint64_t)threadIdx.x * per, ntiles);
    const uint32_t t1 = (uint32_t)std::min<uint64_t>((uint64_t)t0 + per, ntiles);
    uint32_t s = 0;
    for (uint32_t i = t0; i < t1; ++i) s += tile_cnt[i];
    uint32_t sum = 0;
    uint32_t at = view_block_scan(s, part, sum);
    for (uint32_t i = t0; i < t1; ++i) {
        const uint32_t c = tile_cnt[i];
        tile_cnt[i] = at;
        at += c;
    }
    if (threadIdx.x == 0) *total = sum;
}

// The flagged rows, ascending: tile `blockIdx.x` writes its rows from sel[tile_off[tile] - off0] on (off0 != 0: flags4 / tile_off
// point at a later tile of the segment, and the rows are numbered from that tile's first row — a chunk of remove_ids).
__global__ __launch_bounds__(256) void view_compact_kernel(const uint32_t* __restrict__ flags4, const uint32_t* __restrict__ tile_off,
                                                           uint32_t off0, uint32_t* __restrict__ sel) {
    __shared__ uint32_t part[4];
    const uint32_t f = flags4[(size_t)blockIdx.x * 256 + threadIdx.x];
    uint32_t total = 0;
    uint32_t at = tile_off[blockIdx.x] - off0 + view_block_scan((uint32_t)__popc(f), part, total);
    const uint32_t r0 = blockIdx.x * (uint32_t)kViewTile + threadIdx.x * 4u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if ((f >> (8 * j)) & 1u) sel[at++] = r0 + j;
}

// Rows [dst_row0, dst_end) of a view segment: row dst_row0 + i takes row sel[i] of a parent segment for i < n_sel — its 16-byte
// pieces, its scale (0 keeps a hidden or unsearchable row unsearchable), its id (id0 + row for implicit ids) and its parent
// position pos0 + row (dst_ppos[c]) —; the rows after those are padding (zeros, scale 0, id -1).  One thread per piece, as
// pack_rows_kernel: lanes 0..31 are the 32 rows of a block, the two halves of a wave neighbouring pieces, so a wave writes 1 KB
// contiguously (consecutive view rows); the reads are as contiguous as the selected rows are.
__global__ __launch_bounds__(256) void view_gather_kernel(const float4* __restrict__ src_blk, const float* __restrict__ src_scale,
                                                          const int64_t* __restrict__ src_ids, int64_t src_id0, int64_t src_pos0,
                                                          const uint32_t* __restrict__ sel, uint32_t n_sel, int D4, uint32_t dst_row0,
                                                          uint32_t dst_end, float4* __restrict__ dst_blk, float* __restrict__ dst_scale,
                                                          int64_t* __restrict__ dst_ids, int64_t* __restrict__ dst_ppos, int64_t threads) {
    const uint64_t first_blk = dst_row0 >> 5;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < threads; t += (int64_t)gridDim.x * 256) {
        const uint32_t r = (uint32_t)(t & 31);
        const int64_t u = t >> 5;
        const int f4 = (int)(u % D4);
        const uint64_t b = first_blk + (uint64_t)(u / D4);
        const uint64_t c = b * 32 + r;
        if (c < dst_row0 || c >= dst_end) continue;
        const uint32_t i = (uint32_t)(c - dst_row0);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < n_sel) {
            const uint32_t row = sel[i];
            v = src_blk[((size_t)(row >> 5) * D4 + f4) * 32 + (row & 31)];
            if (f4 == 0) {
                dst_scale[c] = src_scale[row];
                dst_ids[c] = src_ids ? src_ids[row] : src_id0 + row;
                if (dst_ppos) dst_ppos[c] = src_pos0 + row;
            }
        } else if (f4 == 0) {
            dst_scale[c] = 0.0f;
            dst_ids[c] = -1;
        }
        dst_blk[(b * D4 + f4) * 32 + r] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// removed items (pcv_searcher_remove_ids, DESIGN.md §3 "Removed items"): a segment is compacted in place, chunk by chunk.  The
// rows of a chunk that stay are marked and listed by the view kernels above (flag = the row stays) and gathered by
// view_gather_kernel into a bounce buffer that already has the blocked layout of their destination; this kernel then writes the
// bounce buffer to the destination.  Two launches in stream order, so no row is overwritten before it has been read.
// ------------------------------------------------------------------------------------------------

// Rows [dst_row0, dst_end) of a segment take the rows of the bounce buffer at the same place inside their blocks: block 0 of the
// bounce buffer stands for block dst_row0 / 32 of the segment.  Pieces, scale and id, bit for bit.  One thread per 16-byte piece,
// lanes 0..31 the rows of a block and the two halves of a wave neighbouring pieces: a wave reads and writes 1 KB contiguously.
// Rows of the first and last block outside [dst_row0, dst_end) are left alone.
__global__ __launch_bounds__(256) void compact_store_kernel(const float4* __restrict__ bounce_blk, const float* __restrict__ bounce_scale,
                                                            const int64_t* __restrict__ bounce_ids, int D4, uint32_t dst_row0,
                                                            uint32_t dst_end, float4* __restrict__ dst_blk, float* __restrict__ dst_scale,
                                                            int64_t* __restrict__ dst_ids, int64_t threads) {
    const uint64_t first_blk = dst_row0 >> 5;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < threads; t += (int64_t)gridDim.x * 256) {
        const uint32_t r = (uint32_t)(t & 31);
        const int64_t u = t >> 5;
        const int f4 = (int)(u % D4);
        const uint64_t lb = (uint64_t)(u / D4);
        const uint64_t c = (first_blk + lb) * 32 + r;
        if (c < dst_row0 || c >= dst_end) continue;
        dst_blk[((first_blk + lb) * D4 + f4) * 32 + r] = bounce_blk[(lb * D4 + f4) * 32 + r];
        if (f4 == 0) {
            dst_scale[c] = bounce_scale[lb * 32 + r];
            dst_ids[c] = bounce_ids[lb * 32 + r];
        }
    }
}

// Hit lists of a view: a position p in [0, nrows) (the view's own numbering) becomes its parent's position ppos[p]; empty slots
// (p < 0) stay.
__global__ __launch_bounds__(256) void view_remap_kernel(pcv_hit_dev* __restrict__ hits, int64_t n, const int64_t* __restrict__ ppos,
                                                         int64_t nrows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t p = hits[i].pos;
    if (p >= 0 && p < nrows) hits[i].pos = ppos[p];
}

struct SynthShape {  // n_clusters == 0: plain i.i.d. rows, times a per-row amplitude in [amp_lo, amp_lo + amp_span) if amp_span >= 0
    uint32_t n_clusters;
    float noise, inv_sqrt_d;
    float amp_lo, amp_span;  // amp_span < 0: no amplitude
};
__device__ __forceinline__ float4 synth_value(uint64_t seed, int64_t row, uint32_t f4, const SynthShape& sh) {
    if (sh.n_clusters) return synth_piece_clustered(seed, row, f4, sh.n_clusters, sh.noise, sh.inv_sqrt_d);
    return sh.amp_span >= 0.0f ? synth_piece_scaled(seed, row, f4, sh.amp_lo, sh.amp_span) : synth_piece(seed, row, f4);
}

__global__ __launch_bounds__(256) void synth_inv_kernel(uint32_t nrows, int D4src, uint64_t seed, int64_t first_row,
                                                        SynthShape sh, float* __restrict__ inv) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x;
    if (row >= nrows) return;
    const double nx = row_sum_squares(D4src, [&](int f4) { return synth_value(seed, first_row + row, (uint32_t)f4, sh); });
    inv[row] = (float)(1.0 / sqrt(nx));
}

// thread per (block, piece, row-in-block), grid-stride (a 100M-row segment has 9.6e9 work items,
// more than one launch dimension can carry): segment rows row0..row0+nrows get synth rows
// first_row.. ; pieces beyond D stay zero
__global__ __launch_bounds__(256) void synth_fill_kernel(float4* __restrict__ blk, uint32_t nrows, uint32_t row0,
                                                         int D4src, int D4, uint64_t seed, int64_t first_row,
                                                         SynthShape sh, const float* __restrict__ inv, int64_t total) {
    const uint32_t first_blk = row0 >> 5;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int r = (int)(t & 31);
        const int64_t u = t >> 5;
        const int f4 = (int)(u % D4src);
        const int64_t lb = u / D4src;
        const int64_t row = (lb + first_blk) * 32 + r;
        const int64_t src = row - row0;
        if (src < 0 || src >= nrows) continue;
        float4 v = synth_value(seed, first_row + src, (uint32_t)f4, sh);
        if (inv) {
            float s = inv[src];
            v.x *= s;
            v.y *= s;
            v.z *= s;
            v.w *= s;
        }
        blk[((lb + first_blk) * D4 + f4) * 32 + r] = v;
    }
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const SegDesc* __restrict__ segs, int nseg,
                                                          const int64_t* __restrict__ pos, int64_t n, int D, int D4,
                                                          float* __restrict__ out_rows,
                                                          int64_t* __restrict__ out_ids) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int D4src = (D + 3) / 4;
    const int64_t i = t / D4src;
    const int f4 = (int)(t % D4src);
    if (i >= n) return;
    const int64_t gp = pos[i];
    int s = -1;
    for (int j = 0; j < nseg; ++j)
        if (gp >= segs[j].pos0 && gp < segs[j].pos0 + (int64_t)segs[j].nrows) s = j;
    float4 v = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
    int64_t id = -1;
    if (s >= 0) {
        const uint32_t row = (uint32_t)(gp - segs[s].pos0);
        v = segs[s].blk[((size_t)(row >> 5) * D4 + f4) * 32 + (row & 31)];
        id = segs[s].ids ? segs[s].ids[row] : segs[s].id0 + row;
    }
    const float vv[4] = {v.x, v.y, v.z, v.w};
    for (int j = 0; j < 4; ++j)
        if (f4 * 4 + j < D) out_rows[i * D + f4 * 4 + j] = vv[j];
    if (f4 == 0 && out_ids) out_ids[i] = id;
}

// Search by example (pcv_searcher_like_queries, DESIGN.md §3 "Search by example"): query q is the weighted sum of the stored f32
// rows members[first[q] .. first[q + 1]), out[q][c] = the f32 value of acc = fmaf(w, x[c], acc) over the members IN THAT ORDER.
// One thread owns one 16-byte piece of one query from the first member to the last: no atomics, no cross-lane reduction, so the
// order and the bits are fixed.  acc starts at -0.0f, the additive identity that keeps the sign of a zero product: one member of
// weight 1 gives back its row bit for bit.  A query without members is +0.  A member outside the table is a host bug: the
// assert fails the launch loudly, and no row outside a segment is read.
__global__ __launch_bounds__(64) void like_queries_kernel(const SegDesc* __restrict__ segs, int nseg,
                                                          const LikeMember* __restrict__ members,
                                                          const uint32_t* __restrict__ first, int D, int D4,
                                                          float* __restrict__ out) {
    const int q = blockIdx.x;
    const int f4 = blockIdx.y * 64 + threadIdx.x;
    if (f4 * 4 >= D) return;
    const uint32_t m0 = first[q], m1 = first[q + 1];
    float acc[4] = {-0.0f, -0.0f, -0.0f, -0.0f};
    for (uint32_t m = m0; m < m1; ++m) {
        const LikeMember e = members[m];
        const bool inside = e.seg < (uint32_t)nseg && e.row < segs[e.seg].nrows;
        assert(inside && "like_queries_kernel: member outside the segment table");
        if (!inside) continue;  // (a build without asserts: still no read out of bounds)
        const float4 v = segs[e.seg].blk[((size_t)(e.row >> 5) * D4 + f4) * 32 + (e.row & 31)];
        acc[0] = __builtin_fmaf(e.w, v.x, acc[0]);
        acc[1] = __builtin_fmaf(e.w, v.y, acc[1]);
        acc[2] = __builtin_fmaf(e.w, v.z, acc[2]);
        acc[3] = __builtin_fmaf(e.w, v.w, acc[3]);
    }
    for (int j = 0; j < 4; ++j)
        if (f4 * 4 + j < D) out[(size_t)q * D + f4 * 4 + j] = m1 > m0 ? acc[j] : 0.0f;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------

void launch_pack_rows(hipStream_t st, const float* rows, int64_t n, int D, int D4, float4* blk, uint32_t row0) {
    if (n <= 0) return;
    const uint32_t first_blk = row0 >> 5;
    const uint32_t last_blk = (uint32_t)((row0 + n - 1) >> 5);
    const int64_t threads = (int64_t)(last_blk - first_blk + 1) * D4 * 32;
    if (threads > (int64_t)0xffffff00u)
        PCV_FAIL(PCV_ERR_INTERNAL, "pack_rows: %lld rows in one staging step (callers stage <= 2^18 rows per call)", (long long)n);
    pack_rows_kernel<<<cdiv64(threads, 256), 256, 0, st>>>(rows, n, D, D4, blk, row0);
    PCV_LAUNCHED();
}

void launch_iota_ids(hipStream_t st, int64_t* ids, int64_t first, int64_t n) {
    if (n <= 0) return;
    iota_ids_kernel<<<cdiv64(n, 256), 256, 0, st>>>(ids, first, n);
    PCV_LAUNCHED();
}

void launch_row_scales(hipStream_t st, const float4* blk, uint32_t first_block, uint32_t nblocks, uint32_t nrows, int D4,
                       int metric, float* scale, uint32_t* max_norm_bits) {
    if (nblocks <= first_block) return;
    const uint32_t r0 = first_block * 32, r1 = nblocks * 32;
    row_scales_kernel<<<cdiv64((int64_t)r1 - r0, 256), 256, 0, st>>>(blk, r0, r1, nrows, D4, metric, scale, max_norm_bits);
    PCV_LAUNCHED();
}

void launch_synth_fill(hipStream_t st, float4* blk, uint32_t nrows, uint32_t row0, int D, int D4, uint64_t seed,
                       int64_t first_row, int normalize, uint32_t n_clusters, float noise, float amp_lo, float amp_hi) {
    if (nrows == 0) return;
    const int D4src = D / 4;
    const SynthShape sh{n_clusters, noise, 1.0f / sqrtf((float)D), amp_lo, amp_hi > amp_lo ? amp_hi - amp_lo : (amp_hi == amp_lo && amp_lo > 0.0f ? 0.0f : -1.0f)};
    float* inv = nullptr;
    if (normalize) {
        PCV_HIP(hipMallocAsync((void**)&inv, (size_t)nrows * sizeof(float), st));
        synth_inv_kernel<<<cdiv64(nrows, 256), 256, 0, st>>>(nrows, D4src, seed, first_row, sh, inv);
    }
    const uint32_t first_blk = row0 >> 5;
    const uint32_t last_blk = (uint32_t)(((uint64_t)row0 + nrows - 1) >> 5);
    const int64_t threads = (int64_t)(last_blk - first_blk + 1) * D4src * 32;
    const unsigned grid = (unsigned)std::min<int64_t>((threads + 255) / 256, 1 << 20);
    synth_fill_kernel<<<grid, 256, 0, st>>>(blk, nrows, row0, D4src, D4, seed, first_row, sh, inv, threads);
    const hipError_t e = hipGetLastError();
    if (inv) (void)hipFreeAsync(inv, st);
    PCV_HIP(e);
}

void launch_gather_rows(hipStream_t st, const SegDesc* d_segs, int nseg, const int64_t* d_pos, int64_t n, int D,
                        int D4, float* out_rows, int64_t* out_ids) {
    if (n <= 0) return;
    const int64_t threads = n * ((D + 3) / 4);
    gather_rows_kernel<<<cdiv64(threads, 256), 256, 0, st>>>(d_segs, nseg, d_pos, n, D, D4, out_rows, out_ids);
    PCV_LAUNCHED();
}

void launch_like_queries(hipStream_t st, const SegDesc* d_segs, int nseg, const LikeMember* d_members, const uint32_t* d_first,
                         int n_queries, int D, int D4, float* out) {
    if (n_queries <= 0) return;
    PCV_REQUIRE(D > 0 && D <= D4 * 4, "like_queries: bad shape (dim %d, %d pieces)", D, D4);  // (grid.x takes any int of queries)
    const dim3 grid((unsigned)n_queries, (unsigned)(((D + 3) / 4 + 63) / 64));
    like_queries_kernel<<<grid, 64, 0, st>>>(d_segs, nseg, d_members, d_first, D, D4, out);
    PCV_LAUNCHED();
}

size_t six_copy_bytes(uint32_t nblocks, int Dp) { return (size_t)nblocks * (size_t)(((Dp + 127) & ~127) >> 7) * 3072; }
void launch_pack6(hipStream_t st, const float4* blk, const float* scale, const uint4* blk8, const float* scale8, uint4* blk6, float4* scale6,
                  uint32_t first_block, uint32_t nblocks, int D4) {
    if (first_block >= nblocks) return;
    pack6_kernel<<<std::min<unsigned>(cdiv64((int64_t)(nblocks - first_block), 4), 1u << 16), 256, 0, st>>>(blk, scale, blk8, scale8, nullptr, blk6, scale6, first_block,
                                                                              nblocks, D4);
    PCV_LAUNCHED();
}
void launch_repack6_blocks(hipStream_t st, const float4* blk, const float* scale, const uint4* blk8, const float* scale8, const uint32_t* blocks,
                           uint32_t n, uint4* blk6, float4* scale6, int D4) {
    if (n == 0) return;
    pack6_kernel<<<std::min<unsigned>(cdiv64((int64_t)n, 4), 1u << 16), 256, 0, st>>>(blk, scale, blk8, scale8, blocks, blk6, scale6, 0u, n, D4);
    PCV_LAUNCHED();
}

void launch_coarse_pack8(hipStream_t st, const float4* blk, const float* scale, uint4* blk8, float* scale8, uint32_t first_block,
                         uint32_t nblocks, int D4) {
    if (first_block >= nblocks) return;
    const unsigned grid = (unsigned)std::min<uint32_t>((nblocks - first_block + 3) / 4, 1u << 16);
    coarse_pack8_kernel<<<grid, 256, 0, st>>>(blk, scale, blk8, scale8, first_block, nblocks, D4);
    PCV_LAUNCHED();
}

void launch_mid_pack(hipStream_t st, const float4* blk, const float* scale, const float* scale8, uint4* mid16, float* scale16,
                     uint32_t first_row, uint32_t nrows, int D4) {
    if (first_row >= nrows) return;
    if (scale8) {  // the segment has its int8 copy (and with it the blocks' maxima): block by block, every row read once
        const uint32_t b0 = first_row / kBlockRows, nb = (nrows + kBlockRows - 1) / kBlockRows;
        const size_t lds = (size_t)32 * (D4 + 2) * sizeof(uint2);
        allow_dynamic_lds((const void*)mid_pack_block_kernel, lds);
        const unsigned per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>(8, (150 * 1024) / lds));
        const unsigned gridb = std::min<uint32_t>(nb - b0, (unsigned)current_device_cus() * per_cu);
        mid_pack_block_kernel<<<gridb, 64, lds, st>>>(blk, scale, scale8, mid16, scale16, b0, nb, D4);
        PCV_LAUNCHED();
        return;
    }
    const unsigned grid = (unsigned)std::min<uint32_t>((nrows - first_row + 3) / 4, 256u * 8 * 4);
    mid_pack_kernel<<<grid, 256, 0, st>>>(blk, scale, mid16, scale16, first_row, nrows, D4);
    PCV_LAUNCHED();
}

void launch_match_ids(hipStream_t st, const int64_t* ids, uint32_t row0, uint32_t row1, const int64_t* table, uint32_t tmask,
                      bool has_empty, uint32_t* out_rows, uint32_t* out_n, uint32_t cap) {
    PCV_HIP(hipMemsetAsync(out_n, 0, sizeof(uint32_t), st));
    if (row0 >= row1) return;
    // enough waves to keep the id stream at HBM rate (8 KB of ids per workgroup and step), each walking a stretch of rows
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64((int64_t)row1 - row0, 256), (int64_t)current_device_cus() * 16);
    match_ids_kernel<<<grid, 256, 0, st>>>(ids, row0, row1, table, tmask, has_empty ? 1 : 0, out_rows, out_n, cap);
    PCV_LAUNCHED();
}

void launch_hide_rows(hipStream_t st, const uint32_t* rows, uint32_t n, float* scale, uint4* blk8, uint4* blk16, uint32_t copied_rows,
                      float* scale16, uint32_t mid_rows, int D4) {
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<uint32_t>((n + 3) / 4, 1u << 16);
    hide_rows_kernel<<<grid, 256, 0, st>>>(rows, n, scale, blk8, blk16, copied_rows, scale16, mid_rows, D4);
    PCV_LAUNCHED();
}

void launch_restore_scales(hipStream_t st, const float4* blk, const uint32_t* rows, uint32_t n, int D4, int metric, float* scale) {
    if (n == 0) return;
    restore_scales_kernel<<<cdiv64(n, 256), 256, 0, st>>>(blk, rows, n, D4, metric, scale);
    PCV_LAUNCHED();
}

void launch_repack8_blocks(hipStream_t st, const float4* blk, const float* scale, const uint32_t* blocks, uint32_t n, uint4* blk8,
                           float* scale8, int D4) {
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<uint32_t>((n + 3) / 4, 1u << 16);
    repack8_blocks_kernel<<<grid, 256, 0, st>>>(blk, scale, blocks, n, blk8, scale8, D4);
    PCV_LAUNCHED();
}

void launch_repack16_rows(hipStream_t st, const float4* blk, const float* scale, const uint32_t* rows, uint32_t n, uint4* blk16, int D4) {
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<uint32_t>((n + 3) / 4, 1u << 16);
    repack16_rows_kernel<<<grid, 256, 0, st>>>(blk, scale, rows, n, blk16, D4);
    PCV_LAUNCHED();
}

void launch_repack_mid(hipStream_t st, const float4* blk, const float* scale, const float* scale8, const uint32_t* items, uint32_t n,
                       uint32_t mid_rows, uint4* mid16, float* scale16, int D4) {
    if (n == 0) return;
    const uint64_t waves = (uint64_t)n * (scale8 ? 32u : 1u);
    const unsigned grid = (unsigned)std::min<uint64_t>((waves + 3) / 4, 1u << 16);
    repack_mid_kernel<<<grid, 256, 0, st>>>(blk, scale, scale8, items, n, mid_rows, mid16, scale16, D4);
    PCV_LAUNCHED();
}

void launch_match_id_slots(hipStream_t st, const int64_t* ids, uint32_t row0, uint32_t row1, const int64_t* table, const uint32_t* vals,
                           uint32_t tmask, bool has_empty, uint32_t empty_slot, uint32_t* out_rows, uint32_t* out_slots,
                           uint32_t* out_n, uint32_t cap) {
    PCV_HIP(hipMemsetAsync(out_n, 0, sizeof(uint32_t), st));
    if (row0 >= row1) return;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64((int64_t)row1 - row0, 256), (int64_t)current_device_cus() * 16);
    match_id_slots_kernel<<<grid, 256, 0, st>>>(ids, row0, row1, table, vals, tmask, has_empty ? 1 : 0, empty_slot, out_rows, out_slots,
                                                out_n, cap);
    PCV_LAUNCHED();
}

void launch_update_rows(hipStream_t st, const float* stage, uint32_t slot0, const uint32_t* rows, const uint32_t* slots, uint32_t n,
                        int D, int D4, int metric, float4* blk, float* scale, uint32_t* max_norm_bits) {
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<uint32_t>((n + 3) / 4, 1u << 16);
    update_rows_kernel<<<grid, 256, 0, st>>>(stage, slot0, rows, slots, n, D, D4, metric, blk, scale, max_norm_bits);
    PCV_LAUNCHED();
}

uint32_t view_tiles(uint32_t nrows) { return (nrows + kViewTile - 1) / kViewTile; }

void launch_view_select(hipStream_t st, const int64_t* ids, uint32_t nrows, const int64_t* table, uint32_t tmask, bool has_empty,
                        uint32_t* flags4, uint32_t* tile_cnt, uint32_t* total, bool invert) {
    const uint32_t nt = view_tiles(nrows);
    if (nt == 0) {
        PCV_HIP(hipMemsetAsync(total, 0, sizeof(uint32_t), st));
        return;
    }
    view_mark_kernel<<<nt, 256, 0, st>>>(ids, nrows, table, tmask, has_empty ? 1 : 0, invert ? 1 : 0, flags4, tile_cnt);
    PCV_LAUNCHED();
    launch_view_scan(st, tile_cnt, nt, total);
}

void launch_view_scan(hipStream_t st, uint32_t* tile_cnt, uint32_t ntiles, uint32_t* total) {
    view_scan_kernel<<<1, 256, 0, st>>>(tile_cnt, ntiles, total);
    PCV_LAUNCHED();
}

void launch_view_compact(hipStream_t st, const uint32_t* flags4, const uint32_t* tile_off, uint32_t nrows, uint32_t* sel, uint32_t off0) {
    const uint32_t nt = view_tiles(nrows);
    if (nt == 0) return;
    view_compact_kernel<<<nt, 256, 0, st>>>(flags4, tile_off, off0, sel);
    PCV_LAUNCHED();
}

void launch_view_gather(hipStream_t st, const float4* src_blk, const float* src_scale, const int64_t* src_ids, int64_t src_id0,
                        int64_t src_pos0, const uint32_t* sel, uint32_t n_sel, int D4, uint32_t dst_row0, uint32_t dst_end,
                        float4* dst_blk, float* dst_scale, int64_t* dst_ids, int64_t* dst_ppos) {
    if (dst_end <= dst_row0) return;
    const uint64_t first_blk = dst_row0 >> 5, last_blk = ((uint64_t)dst_end - 1) >> 5;
    const int64_t threads = (int64_t)(last_blk - first_blk + 1) * D4 * 32;
    const unsigned grid = (unsigned)std::min<int64_t>((threads + 255) / 256, (int64_t)current_device_cus() * 64);
    view_gather_kernel<<<grid, 256, 0, st>>>(src_blk, src_scale, src_ids, src_id0, src_pos0, sel, n_sel, D4, dst_row0, dst_end, dst_blk,
                                             dst_scale, dst_ids, dst_ppos, threads);
    PCV_LAUNCHED();
}

void launch_compact_store(hipStream_t st, const float4* bounce_blk, const float* bounce_scale, const int64_t* bounce_ids, int D4,
                          uint32_t dst_row0, uint32_t dst_end, float4* dst_blk, float* dst_scale, int64_t* dst_ids) {
    if (dst_end <= dst_row0) return;
    const uint64_t first_blk = dst_row0 >> 5, last_blk = ((uint64_t)dst_end - 1) >> 5;
    const int64_t threads = (int64_t)(last_blk - first_blk + 1) * D4 * 32;
    const unsigned grid = (unsigned)std::min<int64_t>((threads + 255) / 256, (int64_t)current_device_cus() * 64);
    compact_store_kernel<<<grid, 256, 0, st>>>(bounce_blk, bounce_scale, bounce_ids, D4, dst_row0, dst_end, dst_blk, dst_scale, dst_ids,
                                               threads);
    PCV_LAUNCHED();
}

void launch_view_remap(hipStream_t st, pcv_hit_dev* hits, int64_t n, const int64_t* ppos, int64_t nrows) {
    if (n <= 0) return;
    view_remap_kernel<<<cdiv64(n, 256), 256, 0, st>>>(hits, n, ppos, nrows);
    PCV_LAUNCHED();
}

void launch_coarse_pack(hipStream_t st, const float4* blk, const float* scale, uint4* blk16, uint32_t first_block, uint32_t nblocks,
                        int D4) {
    if (first_block >= nblocks) return;
    const size_t total = (size_t)(nblocks - first_block) * (D4 >> 1) * 32;
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 1u << 16);
    coarse_pack_kernel<<<grid, 256, 0, st>>>(blk, scale, blk16, first_block, nblocks, D4);
    PCV_LAUNCHED();
}

}  // namespace pcv
