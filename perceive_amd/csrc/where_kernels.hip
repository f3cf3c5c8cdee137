// where_kernels.hip — the kernels that test stored rows against a predicate on the value of their item id (corpus.h "filtered
// search"; DESIGN.md §4 "Item values and filtered search"): the mark step of pcv_searcher_count_where and of a predicate view's
// build, the sum of its tile counts, and the select step of pcv_searcher_search_where.
//
// Nothing here depends on the order in which anything lands: every kernel only READS the value table (plain loads of a table at
// rest: the owner's lock is held around the call), where_mark_kernel writes one word per thread and two per tile, where_sum_kernel
// adds integers, and where_select_kernel's slots come from a ballot and a popcount.
#include "corpus.h"
#include "device_access.h"
#include "launch_rows.h"
#include "scan.h"
#include "value_table.h"

namespace pcv {
namespace {

typedef unsigned long long u64;

// Sum of one value per thread over a 256-thread workgroup, in every thread.  `part`: 4 words of LDS.
__device__ __forceinline__ uint32_t block_sum256(uint32_t v, uint32_t* part) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// The rows of a segment that pass, in view_mark_kernel's layout: flags4[tile * 256 + t] holds the flags of rows tile * kViewTile +
// 4t .. 4t + 3 in bits 0, 8, 16, 24; tile_cnt[tile] = the flagged rows of the tile, tile_live[tile] = those of them with
// scale != 0 (the rows a search could return); rows >= nrows are never flagged.  A row's id is ids ? ids[row] : id0 + row.
// This is a gather into a table that may not fit L2: a thread first has its four ids and then the first slot of all four
// chains in flight before it looks at any of them; a chain that does not end in its first slot (the table is at least half
// empty: about one in four) is then walked by find_slot.  The four values are loaded together likewise.
__global__ __launch_bounds__(256) void where_mark_kernel(const int64_t* __restrict__ ids, int64_t id0, const float* __restrict__ scale,
                                                         uint32_t nrows, const ValueTable t, const WherePred w,
                                                         uint32_t* __restrict__ flags4, uint32_t* __restrict__ tile_cnt,
                                                         uint32_t* __restrict__ tile_live) {
    __shared__ uint32_t part[4];
    const uint64_t r0 = (uint64_t)blockIdx.x * kViewTile + threadIdx.x * 4u;
    int64_t id[4], k[4], v[4];
    uint32_t h[4];
    float sc[4];
    bool in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        in[j] = r0 + j < nrows;
        const uint64_t row = in[j] ? r0 + j : (uint64_t)nrows - 1;  // (a row past the end reads the last one and is dropped)
        id[j] = ids ? __builtin_nontemporal_load(&ids[row]) : id0 + (int64_t)row;
        sc[j] = gld(&scale[row]);
    }
    const bool slots = t.keys != nullptr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        h[j] = id_hash(id[j], t.mask);
        k[j] = slots && id[j] != kIdEmpty ? gld(&t.keys[h[j]]) : kIdEmpty;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (k[j] != id[j] && k[j] != kIdEmpty) {
            h[j] = find_slot(t.keys, t.mask, id[j]);
            k[j] = gld(&t.keys[h[j]]);
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = id[j] == kIdEmpty ? t.side_val : (k[j] == id[j] ? gld(&t.vals[h[j]]) : kNoValue);
    uint32_t f = 0, live = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (in[j] && where_passes(v[j], w)) {
            f |= 1u << (8 * j);
            live += sc[j] != 0.0f ? 1u : 0u;
        }
    flags4[(size_t)blockIdx.x * 256 + threadIdx.x] = f;
    const uint32_t both = block_sum256((uint32_t)__popc(f) | (live << 16), part);  // (at most kViewTile = 1024 each: 16 bits hold it)
    if (threadIdx.x == 0) {
        tile_cnt[blockIdx.x] = both & 0xffffu;
        tile_live[blockIdx.x] = both >> 16;
    }
}

// acc[0] += the sum of tile_cnt, acc[1] += the sum of tile_live: one workgroup, launches of one stream follow each other.
__global__ __launch_bounds__(256) void where_sum_kernel(const uint32_t* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_live,
                                                        uint32_t ntiles, int64_t* __restrict__ acc) {
    __shared__ u64 part[2][4];
    u64 a = 0, b = 0;
    for (uint32_t i = threadIdx.x; i < ntiles; i += 256) {
        a += gld(&tile_cnt[i]);
        b += gld(&tile_live[i]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a += shfl_xor_u64(a, d);
        b += shfl_xor_u64(b, d);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = a;
        part[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const u64 sum = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        gst(&acc[threadIdx.x], gld(&acc[threadIdx.x]) + (int64_t)sum);
    }
}

// The select step: one workgroup of kMaxK threads per query, thread t for hit t of the pass's list (p.out, best first; the hits
// of a short list come first).  Hit t is kept iff the value of its id passes.  The passing hits, in list order, are the kept rows of
// this pass: a ballot and a popcount across the two waves give each its output slot, and the one that fills slot num_results - 1 is
// the cut — the walk ends with it, and the hits behind it are not examined.  The record is written as grouped_select_kernel
// writes it.
__global__ __launch_bounds__(kMaxK) void where_select_kernel(const ScanParams* __restrict__ pp, const WhereArgs a) {
    const ScanParams& p = *pp;
    __shared__ u64 s_pass[kMaxK / 64];  // the waves' masks of passing hits ...
    __shared__ u64 s_live[kMaxK / 64];  // ... and of hits at all
    __shared__ int32_t s_cut;
    const int q = blockIdx.x, t = threadIdx.x, n_list = p.k;
    const DistinctRec rec = a.rec[q];
    if (rec.flags != 0) {  // finished in an earlier pass: nothing of it changes
        if (t == 0) a.rec_host[q] = rec;
        return;
    }
    const size_t o = (size_t)q * kMaxK;
    const int nk0 = (int)rec.kept;
    pcv_hit_dev h;
    h.pos = -1;
    if (t < n_list) h = p.out[(size_t)q * n_list + t];
    const bool live = h.pos >= 0;
    const int64_t v = live ? value_of(a.table, h.id) : kNoValue;
    const bool pass = live && where_passes(v, a.where);
    const u64 mask = __ballot(pass), lmask = __ballot(live);
    const int lane = t & 63, wave = t >> 6;
    if (lane == 0) {
        s_pass[wave] = mask;
        s_live[wave] = lmask;
    }
    if (t == 0) s_cut = -1;
    __syncthreads();
    int slot = nk0 + __popcll(mask & (((u64)1 << lane) - 1));
    int n_pass = 0, n_live = 0;
#pragma unroll
    for (int w = 0; w < kMaxK / 64; ++w) {
        const int c = __popcll(s_pass[w]);
        slot += w < wave ? c : 0;
        n_pass += c;
        n_live += __popcll(s_live[w]);
    }
    if (pass && slot == a.num_results - 1) s_cut = t;  // (one hit has that slot, or none)
    __syncthreads();
    const int cut = s_cut;                         // -1: the list ends before the num_results-th kept row
    const int last = cut >= 0 ? cut : n_live - 1;  // the last hit examined (-1: the list was empty)
    if (pass && t <= last) {                       // (slot <= num_results - 1 < kMaxK: up to the cut, or all of too few)
        a.kept[o + slot] = h;
        gst(&a.kept_value[o + slot], v);
    }
    if (t == max(last, 0)) {
        DistinctRec out;
        out.kept = (uint32_t)(cut >= 0 ? a.num_results : nk0 + n_pass);
        out.examined = rec.examined + (uint32_t)(last + 1);
        out.flags = cut >= 0 ? kDistinctFull : (n_live < n_list ? kDistinctEnd : 0u);  // a short list: the query has all the rows there are
        out.pad = 0;
        out.last_score = last >= 0 ? h.score : rec.last_score;
        out.last_pos = last >= 0 ? h.pos : rec.last_pos;
        a.rec[q] = out;
        a.rec_host[q] = out;
    }
}

}  // namespace

void launch_where_mark(hipStream_t st, const int64_t* ids, int64_t id0, const float* scale, uint32_t nrows, const ValueTable& t,
                       const WherePred& w, uint32_t* flags4, uint32_t* tile_cnt, uint32_t* tile_live) {
    const uint32_t nt = view_tiles(nrows);
    if (nt == 0) return;
    PCV_REQUIRE(scale != nullptr && (t.keys == nullptr || (t.vals != nullptr && (t.mask & (t.mask + 1)) == 0)),
                "where mark: bad shape (%u rows, mask %#x)", nrows, t.mask);
    where_mark_kernel<<<nt, 256, 0, st>>>(ids, id0, scale, nrows, t, w, flags4, tile_cnt, tile_live);
    PCV_LAUNCHED();
}

void launch_where_sum(hipStream_t st, const uint32_t* tile_cnt, const uint32_t* tile_live, uint32_t ntiles, int64_t* acc) {
    if (ntiles == 0) return;
    where_sum_kernel<<<1, 256, 0, st>>>(tile_cnt, tile_live, ntiles, acc);
    PCV_LAUNCHED();
}

void launch_where_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const WhereArgs& a) {
    PCV_REQUIRE(p.B > 0 && p.k >= 1 && p.k <= kMaxK && a.num_results >= 1 && a.num_results <= kMaxK,
                "where select: bad shape (%d queries, lists of %d, %d results)", p.B, p.k, a.num_results);
    PCV_REQUIRE(a.table.keys == nullptr || (a.table.mask & (a.table.mask + 1)) == 0, "where select: mask %#x", a.table.mask);
    where_select_kernel<<<p.B, kMaxK, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

}  // namespace pcv
