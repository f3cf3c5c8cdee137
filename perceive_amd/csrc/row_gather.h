// row_gather.h — hit rows out of the blocked layout: where a row starts, and the four-rows-in-flight gather.  Shared by the select
// steps that compare rows with rows (distinct_kernels.hip, diverse_kernels.hip).  Everything here is inlined: no symbol.
#pragma once
#include "device_access.h"
#include "scan.h"

namespace pcv {
namespace {

// Row `pos` (a global position, as a hit carries it) in the segments of the pass: the address of its first piece.
__device__ __forceinline__ uint64_t row_start(const ScanParams& p, int64_t pos) {
    for (int i = 0; i < p.nseg; ++i) {
        const SegDesc& sg = p.seg[i];
        const int64_t pos0 = gld(&sg.pos0);
        const uint32_t nrows = gld(&sg.nrows);
        if (pos >= pos0 && pos < pos0 + (int64_t)nrows) {
            const uint32_t row = (uint32_t)(pos - pos0);
            return (uint64_t)(gld(&sg.blk) + (size_t)(row >> 5) * p.D4 * 32 + (row & 31));
        }
    }
    return 0;
}

// n rows into a tile (piece f of row r at tile[r * row_pitch + f * piece_pitch]; 256 threads): a wave takes rows wave, wave + 4,
// ...; four rows' pieces are requested before any is stored.  A row that starts at 0 is stored as zeros.
__device__ __forceinline__ void stage_rows(float4* tile, size_t row_pitch, size_t piece_pitch, const uint64_t* src, int n, int D4, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    for (int r0 = wave; r0 < n; r0 += 16) {
        for (int f = lane; f < D4; f += 64) {
            float4 t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = r0 + 4 * u;
                const float4* s = r < n ? (const float4*)src[r] : nullptr;
                t[u] = s ? gld4(s + (size_t)f * 32) : make_float4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = r0 + 4 * u;
                if (r < n) tile[(size_t)r * row_pitch + (size_t)f * piece_pitch] = t[u];
            }
        }
    }
}
// ... into an LDS tile of row pitch D4 + 1 pieces (a lane's 16-byte reads of different rows fall into different banks)
__device__ __forceinline__ void stage_rows(float4* tile, const uint64_t* src, int n, int D4, int tid) {
    stage_rows(tile, (size_t)D4 + 1, 1, src, n, D4, tid);
}

}  // namespace
}  // namespace pcv
