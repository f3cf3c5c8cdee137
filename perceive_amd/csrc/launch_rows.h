// launch_rows.h — what the kernels that walk a launch's rows by number share: finding the segment of a launch row (row_jobs.h,
// "launch row") and its id, the wave-uniform cursor of a stream of row blocks (pair_screen.h streams with it), the 64-bit atomics and
// the lock-free union-find over launch rows.  Everything here is inlined: the file defines no symbol.
#pragma once
#include "device_access.h"
#include "row_jobs.h"

namespace pcv {
namespace {

__device__ __forceinline__ unsigned long long g_atomic_add64(unsigned long long* p, unsigned long long v) {
    return __hip_atomic_fetch_add((PCV_GLOBAL unsigned long long*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void g_atomic_max64(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_max((PCV_GLOBAL unsigned long long*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void g_atomic_min64(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_min((PCV_GLOBAL unsigned long long*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void g_atomic_add_i64(long long* p, long long v) {
    (void)__hip_atomic_fetch_add((PCV_GLOBAL long long*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The fixed-point unit row (perceive_hip.h, pcv_searcher_label_sums): t(r, d) = unit_int(x[r][d], unit_scale(|x_r|^2)) — the f32 rinv
// of the prep step (also where that marks a row wild) times 2^32, exact; the product of two f32 is exact in f64, so rint is the one
// rounding.  The one copy of this arithmetic: label_sums_kernel and the kernels of moments_kernels.hip call it.
__device__ __forceinline__ bool has_cosine(double n) { return n >= 0x1p-126 && n < __builtin_inf(); }
__device__ __forceinline__ double unit_scale(double n) { return (double)(float)(1.0 / sqrt(n)) * 0x1p32; }
__device__ __forceinline__ long long unit_int(float x, double rs) { return (long long)rint((double)x * rs); }

// last table entry with blk0 <= gb
__device__ __forceinline__ int find_seg(const ScanParams& p, uint32_t gb, int from = 0) {
    int lo = from, hi = p.nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (gld(&p.seg[mid].blk0) <= gb)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// Launch row `lr` (row_jobs.h): its segment, its row there and where its first piece is.
struct RowRef {
    const SegDesc* sg;
    uint32_t row;
    const float4* x;
};
__device__ __forceinline__ RowRef row_ref(const ScanParams& p, uint32_t lr) {
    const uint32_t gb = lr >> 5;
    const SegDesc* sg = &p.seg[find_seg(p, gb)];
    const uint32_t lb = gb - gld(&sg->blk0);
    return {sg, lb * 32 + (lr & 31), gld(&sg->blk) + (size_t)lb * p.D4 * 32 + (lr & 31)};
}

// the id of the row: its segment's list, or consecutive ids from the segment's first
__device__ __forceinline__ int64_t row_id(const RowRef& r) {
    const int64_t* ids = gld(&r.sg->ids);
    return ids ? gld(&ids[r.row]) : gld(&r.sg->id0) + (int64_t)r.row;
}

// The root of x in a forest over launch rows: parents are read with agent-scope atomic loads (other workgroups hook roots while this
// one walks).  parent[r] <= r for every r at every time, so the walk visits strictly descending rows and ends.  A stale answer — a row
// that was a root when it was read and is hooked by now — is caught by the compare-and-swap of the caller.
__device__ __forceinline__ uint32_t row_find(const uint32_t* parent, uint32_t x) {
    while (true) {
        const uint32_t q = ld_relaxed(&parent[x]);
        if (q == x) return x;
        x = q;
    }
}

// Lock-free union of the components of a and b: find both roots, hook the larger under the smaller with a compare-and-swap on
// parent[larger] that expects it to still be a root; if it is not, go on from the value the CAS returned (its new parent, a lower
// row).  No path compression, no plain store to `parent` while the calling kernel runs.
// Termination: nothing here waits for a store of another wave.  A parent is only ever replaced by a lower row (a root r gets
// parent[r] < r, and a hooked row is never written again), so every find ends after at most r steps; and a CAS fails only because
// another CAS succeeded on that row, of which there are fewer than the number of rows in the whole launch.  Every loop therefore ends
// by its own CAS succeeding or by finding equal roots, whatever the other waves do — also if they stop.
// The result is the partition into connected components whatever the order: a successful CAS merges exactly the two components
// whose roots it saw, and the loop does not return before a and b have one root.
__device__ __forceinline__ void row_union(uint32_t* parent, uint32_t a, uint32_t b) {
    while (true) {
        a = row_find(parent, a);
        b = row_find(parent, b);
        if (a == b) return;
        if (a > b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t found = g_atomic_cas(&parent[b], b, a);
        if (found == b) return;
        b = found;
    }
}

// The segment a wave's stream is in (all of it wave-uniform, in scalar registers: scan_kernels.hip, seek_seg).
struct JoinSeg {
    int si = -1;
    uint32_t begin = 0, end = 0;
    const float4* blk = nullptr;
};
__device__ __forceinline__ void join_seek(const ScanParams& p, JoinSeg& c, uint32_t gb) {
    if (gb < c.end) return;
    const int lo = find_seg(p, gb, c.si + 1);
    c.si = lo;
    c.begin = uniform(gld(&p.seg[lo].blk0));
    c.end = c.begin + uniform(gld(&p.seg[lo].nblocks));
    c.blk = uniform_ptr(gld(&p.seg[lo].blk));
}
struct JoinCursor {
    uint32_t gb;
    int ch;
    JoinSeg sc;
    __amdgpu_buffer_rsrc_t rows;
};

}  // namespace
}  // namespace pcv
