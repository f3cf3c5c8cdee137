// device_access.h — the small device accessors and vector types the kernel files (scan_kernels.hip, corpus_kernels.hip) share
// (among them the one copy of the canonical score's last step), and the two host helpers of their launchers.  Everything here is inlined: the file defines no symbol.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace pcv {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Every pointer the kernels follow comes out of a struct in memory, so the compiler only knows it
// as a generic ("flat") address.  flat_load/flat_atomic count on BOTH vmcnt and lgkmcnt and return
// out of order: every LDS wait then has to drain the corpus prefetch as well.  All global traffic
// therefore goes through these address-space(1) accessors (global_load / global_store / global_atomic).
#define PCV_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ T gld(const T* p) {
    return *(const PCV_GLOBAL T*)p;
}
template <class T>
__device__ __forceinline__ void gst(T* p, T v) {
    *(PCV_GLOBAL T*)p = v;
}
__device__ __forceinline__ float4 gld4(const float4* p) {
    const f32x4 v = *(const PCV_GLOBAL f32x4*)p;
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float4 gld4(const float* p) { return gld4((const float4*)p); }
__device__ __forceinline__ uint32_t g_atomic_add(uint32_t* p, uint32_t v) {
    return __hip_atomic_fetch_add((PCV_GLOBAL uint32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t g_atomic_max(uint32_t* p, uint32_t v) {
    return __hip_atomic_fetch_max((PCV_GLOBAL uint32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// returns the value found (== expected on success)
__device__ __forceinline__ uint32_t g_atomic_cas(uint32_t* p, uint32_t expected, uint32_t desired) {
    __hip_atomic_compare_exchange_strong((PCV_GLOBAL uint32_t*)p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    return expected;
}
__device__ __forceinline__ uint32_t ld_relaxed(const uint32_t* p) {
    return __hip_atomic_load((const PCV_GLOBAL uint32_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_relaxed(uint32_t* p, uint32_t v) {
    __hip_atomic_store((PCV_GLOBAL uint32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// corpus rows are read exactly once per scan: optionally mark the loads non-temporal
template <bool NTL>
__device__ __forceinline__ float4 ld_row(const float4* p) {
    if constexpr (NTL) {
        const f32x4 v = __builtin_nontemporal_load((const PCV_GLOBAL f32x4*)p);
        return make_float4(v.x, v.y, v.z, v.w);
    } else {
        return gld4(p);
    }
}

// Streamed row chunks are read through a buffer descriptor (four scalar registers: the block's base, wave-uniform) with the
// lane's own byte offset — one vector register that never changes — and a scalar chunk offset: no 64-bit address arithmetic
// in vector registers.  (The compiler did that arithmetic in the registers of a chunk buffer; overwriting a register that a
// load may still be writing costs an s_waitcnt vmcnt(0), i.e. every chunk in flight, per block.)  Loads past `bytes` return 0.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const void* ubase, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)ubase, 0, bytes, 0x00020000);
}
template <bool NTL>
__device__ __forceinline__ float4 ld_piece(__amdgpu_buffer_rsrc_t rsrc, uint32_t lane_bytes, uint32_t chunk_bytes) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_bytes, chunk_bytes, NTL ? 2 : 0);  // aux 2 = nt
    return __builtin_bit_cast(float4, v);
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int off) {
    const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
template <class T>
__device__ __forceinline__ const T* uniform_ptr(const T* ptr) {  // a wave-uniform pointer, moved to scalar registers
    const uint64_t v = (uint64_t)ptr;
    return (const T*)(((uint64_t)uniform((uint32_t)(v >> 32)) << 32) | uniform((uint32_t)v));
}

// the canonical order of two rows: descending score, ties -> lower global position
__device__ __forceinline__ bool better(double sa, int64_t pa, double sb, int64_t pb) {
    return sa > sb || (sa == sb && pa < pb);
}

// canonical score from the two feature-order f64 sums (oracle/scan.c:orc_canonical_score); NaN: undefined
__device__ __forceinline__ double finish_score(int metric, double dot, double nx, double nq) {
    const double inf = __builtin_inf();
    if (metric == PCV_METRIC_DOT) return (dot < inf && dot > -inf && nq < inf) ? dot : __builtin_nan("");
    if (nq >= 0x1p-126 && nq < inf && nx >= 0x1p-126 && nx < inf) {
        const double cc = dot / (sqrt(nq) * sqrt(nx));
        if (cc < inf && cc > -inf) return cc;
    }
    return __builtin_nan("");
}

// relevance of a row from its canonical score (diverse and boosted results): cosine c; dot c / dim, one f64 division
__device__ __forceinline__ double relevance(int metric, int D, double c) { return metric == PCV_METRIC_DOT ? c / (double)D : c; }

// Place of 16-byte piece `pc` of query row `q` inside the row's P8 pieces of the LDS tile: XOR with the row number
// inside groups of 16 pieces, so that the 16 lanes of a ds_read_b128 group (16 consecutive rows, one piece index) hit 16
// distinct bank quads.  P8 is a multiple of 8 (dimension padded to 64), not always of 16: a trailing group of 8 pieces is
// swizzled inside itself (2-way conflicts there; XOR with four bits would leave the row).
__device__ __forceinline__ int swizzle_piece(int pc, int q, int P8) {
    return pc < (P8 & ~15) ? ((pc & ~15) | ((pc ^ q) & 15)) : ((pc & ~7) | ((pc ^ q) & 7));
}

// The feature-order f64 sums of row x with rows y[0..NU) (D4 pieces of four features each, those of x `xstride` float4 apart and
// those of every y `ystride`): the canonical dot product and, for y == x, the canonical |x|^2.  The product of two f32 is exact
// in f64, so every step is one rounding.
template <int NU>
__device__ __forceinline__ void pair_sums(const float4* x, size_t xstride, const float4* (&y)[NU], size_t ystride, int D4, double (&acc)[NU]) {
#pragma unroll
    for (int u = 0; u < NU; ++u) acc[u] = 0.0;
#pragma unroll 4
    for (int f = 0; f < D4; ++f) {
        const float4 v = x[(size_t)f * xstride];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const float4 w = y[u][(size_t)f * ystride];
            acc[u] += (double)v.x * (double)w.x;
            acc[u] += (double)v.y * (double)w.y;
            acc[u] += (double)v.z * (double)w.z;
            acc[u] += (double)v.w * (double)w.w;
        }
    }
}
// ... both sides `stride` apart
template <int NU>
__device__ __forceinline__ void pair_sums(const float4* x, const float4* (&y)[NU], int D4, double (&acc)[NU], size_t stride = 1) {
    pair_sums<NU>(x, stride, y, stride, D4, acc);
}

}  // namespace

static inline unsigned cdiv64(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }
#define PCV_LAUNCHED() PCV_HIP(hipGetLastError())

}  // namespace pcv
