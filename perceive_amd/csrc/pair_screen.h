// pair_screen.h — the row-pair screen (DESIGN.md §4 "The row-pair screen"): the one copy of what the six "row against row" kernels
// share.  A workgroup of kScreenWaves waves stages a tile of NT row blocks in LDS as swizzled bf16 (pair_stage_tile); each wave then
// streams launch blocks out of the blocked f32 layout, rounds a lane's 16-byte pieces to bf16 on the way — the A fragment of
// v_mfma_f32_32x32x16_bf16 — and hands the finished 32 x (32 NT) products of every block to a policy (pair_stream).
// D[row of the streamed block][row of the tile]: lane (c = lane & 31, h = lane >> 5) holds tile rows 32 t + c and, in accumulator i,
// block row (i & 3) + 8 (i >> 2) + 4 h.  Everything here is inlined: the file defines no symbol.
//
// A policy is a plain struct whose members are all __device__ __forceinline__:
//   begin(tb0, c)               the per-tile-row values it keeps beside ra (thresholds, components, ...)
//   prefetch(gb, h, j)          per-block loads beside rb[j] (j = 0..3), issued with it: one chunk ahead of the epilogue, before that
//                               step's row loads
//   block(acc, ra, rb, where)   the epilogue of one streamed block
//   end(ra, c, h)               the publish when the wave's stream has ended
#pragma once
#include "device_access.h"
#include "launch_rows.h"

namespace pcv {
namespace {

constexpr int kScreenWaves = 8;  // waves of a screen workgroup: one tile in LDS per CU, two waves per SIMD

// Where an epilogue is: the tile's first block, the streamed block and the lane.
struct PairWhere {
    uint32_t tb0, gb;
    int c, h;
    __device__ __forceinline__ uint32_t owner_row(int t) const { return (tb0 + t) * 32u + (uint32_t)c; }
    __device__ __forceinline__ uint32_t partner_row(int i) const { return gb * 32u + (uint32_t)((i & 3) + 8 * (i >> 2) + 4 * h); }
};

// The tile: blocks [tb0, tb0 + NT) of the launch (zero rows behind its last block) into lq, [NT*32][Dp/8] 16-byte pieces of 8 bf16,
// swizzled.  The whole workgroup calls it; tbase is NT pointers of static LDS.  The tile is staged when it returns.
template <int NT>
__device__ __forceinline__ void pair_stage_tile(const ScanParams& p, uint4* lq, const float4** tbase, uint32_t tb0) {
    const int D4 = p.D4, P8 = D4 >> 1;
    if (threadIdx.x < NT) {
        const uint32_t gb = tb0 + threadIdx.x;
        const float4* base = nullptr;
        if (gb < p.total_blocks) {
            const SegDesc& sg = p.seg[find_seg(p, gb)];
            base = gld(&sg.blk) + (size_t)(gb - gld(&sg.blk0)) * D4 * 32;
        }
        tbase[threadIdx.x] = base;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NT * 32 * P8; i += kScreenWaves * 64) {
        const int r = i & 31, rest = i >> 5;
        const int tb = rest / P8, pc = rest - tb * P8;
        const float4* base = tbase[tb];
        bf16x8 v8 = {};
        if (base) {
            const float4 lo = gld4(base + (size_t)(2 * pc) * 32 + r), hi = gld4(base + (size_t)(2 * pc + 1) * 32 + r);
            const f32x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            v8 = __builtin_convertvector(v, bf16x8);
        }
        const int row = tb * 32 + r;
        lq[row * P8 + swizzle_piece(pc, row, P8)] = __builtin_bit_cast(uint4, v8);
    }
    __syncthreads();
}

// The stream of one wave: the launch blocks first, first + step, ... below b1 (first < b1; no workgroup barrier in here).  rinv gives
// rb, the 1/|x| of the streamed rows, and — RA — ra, that of the lane's tile rows (zero behind the launch's last block); a kernel whose
// tile does not hold launch rows (assign_screen_kernel) passes RA = false and gets zeros.
template <int NT, bool RA = true, class Policy>
__device__ __forceinline__ void pair_stream(const ScanParams& p, const uint4* lq, const float* rinv, uint32_t tb0, uint32_t first, uint32_t b1,
                                            uint32_t step, Policy& pol) {
    const int D4 = p.D4, P8 = D4 >> 1, NCH = D4 >> 4;
    const int lane = threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;
    float ra[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) ra[t] = RA ? gld(&rinv[(size_t)(tb0 + t) * 32 + c]) : 0.0f;
    pol.begin(tb0, c);

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

    auto enter_block = [&](JoinCursor& k, uint32_t gb) {
        k.gb = gb;
        k.ch = 0;
        if (gb < b1) {
            join_seek(p, k.sc, gb);
            k.rows = row_rsrc(k.sc.blk + (size_t)(gb - k.sc.begin) * D4 * 32, (uint32_t)D4 * 512u);
        }
    };
    const uint32_t lane_off = (uint32_t)(h * 64 + c) * 16u;  // the lane's bytes inside a block
    JoinCursor cons, prod;
    enter_block(cons, first);
    prod = cons;

    float4 buf[2][8];
    // (always issues its loads: past the end of the wave's stream they read a chunk of its last block again — scan_mfma_kernel)
    auto produce = [&](float4 (&b)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) b[i] = ld_piece<false>(prod.rows, lane_off + (uint32_t)((i >> 1) * 4 + (i & 1)) * 512u, (uint32_t)prod.ch * 8192u);
        if (prod.gb < b1 && ++prod.ch == NCH) enter_block(prod, prod.gb + step);
    };

    f32x4 rb[4];  // rinv of the block's rows 8 j + 4 h + (0..3): accumulators 4 j + (0..3)
    auto rb_prefetch = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            rb[j] = *(const PCV_GLOBAL f32x4*)(rinv + (size_t)cons.gb * 32 + 8 * j + 4 * h);
            pol.prefetch(cons.gb, h, j);
        }
    };

    auto consume = [&](const float4 (&b)[8]) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const f32x8 v = {b[2 * ks].x, b[2 * ks].y, b[2 * ks].z, b[2 * ks].w, b[2 * ks + 1].x, b[2 * ks + 1].y, b[2 * ks + 1].z, b[2 * ks + 1].w};
            const bf16x8 av = __builtin_convertvector(v, bf16x8);
            const int pc = 2 * (cons.ch * 4 + ks) + h;
            const int ph = swizzle_piece(pc, c, P8);  // (tile row 32 t + c: the same low four bits as c)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const bf16x8 q8 = *(const bf16x8*)&lq[(32 * t + c) * P8 + ph];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, q8, acc[t], 0, 0, 0);
            }
        }
        if (++cons.ch == NCH) {
            if (NCH < 2) rb_prefetch();
            pol.block(acc, ra, rb, PairWhere{tb0, cons.gb, c, h});
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
            enter_block(cons, cons.gb + step);
        }
    };

    // one chunk of loads in flight while one feeds the matrix cores (every buf[] index a literal, or the array moves to scratch);
    // the block's rinv values are requested one chunk ahead of the epilogue and before that step's row loads
#define PCV_PAIR_STEP(REFILL, CONS)                      \
    if (NCH >= 2 && cons.ch == NCH - 2) rb_prefetch();   \
    produce(buf[REFILL]);                                \
    consume(buf[CONS]);                                  \
    if (cons.gb >= b1) break;
    produce(buf[0]);
    while (true) {
        PCV_PAIR_STEP(1, 0)
        PCV_PAIR_STEP(0, 1)
    }
#undef PCV_PAIR_STEP
    pol.end(ra, c, h);
}

}  // namespace
}  // namespace pcv
