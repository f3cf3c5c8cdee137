// assign_kernels.hip — the device steps of pcv_searcher_assign, _label_sums and _kmeans (DESIGN.md §4 "Item labels"): the best of K
// label vectors for every row, exact, and the integer sum of the unit rows of every label.  The transpose of a search: the reduction
// runs across the LDS tile (the labels), not along the stream (the rows).
//
//   prep     the labels are a small corpus in the blocked f32 layout, so selfjoin_prep_kernel gives their canonical |l|^2 and rinv as
//            it gives the rows' (launch_selfjoin_prep, called twice); assign_labels_kernel then writes each label's screening
//            constants (w, mg: scan.h, AssignArgs) and its bf16 pieces in the swizzled order of the LDS tile.
//   screen   assign_screen_kernel: a workgroup stages one label tile in LDS and its waves stream row blocks out of the blocked f32
//            layout as the A fragment of v_mfma_f32_32x32x16_bf16 (pair_stream of pair_screen.h: DESIGN.md §4 "The row-pair screen").  Per block the
//            epilogue reduces s - mg over the tile's labels for each of the 32 rows, joins it with the bound the earlier tiles left
//            (lb) and lists every (row, label) with s + mg >= that bound.
//   rescore  assign_rescore_kernel: the canonical f64 score of every candidate that passes the FINAL bound (pair_sums, finish_score:
//            the arithmetic of selfjoin_rescore_kernel) and an atomic max of its order-preserving image per row;
//            assign_pick_kernel: an atomic min of the label among the candidates that reach that maximum — (c descending, label
//            ascending), whatever order the atomics land in;  assign_finish_kernel: labels, reported scores, ids, counts.
//   sums     label_sums_kernel: S[label][d] += rint(x[r][d] * rinv_r * 2^32) in int64 — associative, so any order gives the same bits.
//   top-m    pcv_searcher_assign_top (DESIGN.md §4 "Top-m labels"): the same prep, then two passes per label tile through
//            assign_top_screen_kernel — a bound pass that stores each lane column's maximum of s - mg, merged into the row's eight
//            largest by assign_top_merge_kernel, and a list pass against the final thresholds — the f64 step into per-row stretches
//            (assign_top_rescore_kernel behind the neighbours' count and offsets steps) and assign_top_select_kernel.
#include "device_access.h"
#include "launch_rows.h"
#include "pair_screen.h"
#include "row_jobs.h"

namespace pcv {
namespace {

__device__ __forceinline__ uint32_t g_atomic_min(uint32_t* p, uint32_t v) {
    return __hip_atomic_fetch_min((PCV_GLOBAL uint32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread per (label slot, 16-byte piece of 8 bf16); the thread of piece 0 also writes the label's constants
__global__ __launch_bounds__(256) void assign_labels_kernel(const AssignArgs a, int D4) {
    const int P8 = D4 >> 1;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)a.label_blocks * 32 * P8) return;
    const uint32_t slot = (uint32_t)(i / P8);
    const int pc = (int)(i - (uint64_t)slot * P8);
    const float4* base = a.lab_blk + (size_t)(slot >> 5) * D4 * 32 + (slot & 31);
    const float4 lo = gld4(base + (size_t)(2 * pc) * 32), hi = gld4(base + (size_t)(2 * pc + 1) * 32);
    const f32x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const bf16x8 v8 = __builtin_convertvector(v, bf16x8);  // round to nearest even, as the screens round the rows
    a.lab_tile[(size_t)slot * P8 + swizzle_piece(pc, (int)slot, P8)] = __builtin_bit_cast(uint4, v8);
    if (pc != 0) return;
    const float rinv = gld(&a.lab_rinv[slot]);
    float w = rinv, mg = a.margin;
    if (a.metric == PCV_METRIC_DOT) {
        const double n = gld(&a.lab_norm[slot]);
        if ((int)slot >= a.K) {
            w = 0.0f;
        } else if (rinv > 0.0f || n == 0.0) {  // (the zero label: every product is an exact zero)
            w = 1.0f;
            mg = __double2float_ru((double)a.margin * sqrt(n) * (1.0 + 0x1p-40));
        } else {
            w = kRinvWild;
        }
    }
    gst(&a.w[slot], w);
    gst(&a.mg[slot], mg);
}

// one thread per launch row: the state an assignment starts from
__global__ __launch_bounds__(256) void assign_begin_kernel(const ScanParams* __restrict__ pp, const AssignArgs a) {
    const ScanParams& p = *pp;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)p.total_blocks * 32) return;
    gst(&a.lb[i], -__builtin_inff());
    gst(&a.best_key[i], 0ull);
    gst(&a.best_lab[i], 0xffffffffu);
    if (a.metric == PCV_METRIC_DOT && gld(&a.rinv[i]) == 0.0f) {  // no cosine, but its dot products are defined: the f64 step decides
        const RowRef r = row_ref(p, (uint32_t)i);
        if (r.row < gld(&r.sg->nrows) && gld(&gld(&r.sg->scale)[r.row]) != 0.0f) gst(&a.rinv[i], kRinvWild);
    }
}

// The epilogue of the label screen.  The tile holds labels, not launch rows: l0 is its first label, w and mg the screening constants of
// the lane's labels 32 t + c, lbv the carried bound of the streamed block's rows beside rb.  ra is not used.
template <int NT>
struct AssignPolicy {
    const AssignArgs& a;
    uint32_t l0;
    float w[NT], mg[NT];
    f32x4 lbv[4];
    __device__ __forceinline__ void begin(uint32_t, int c) {
        l0 = a.tile * NT * 32;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            w[t] = gld(&a.w[l0 + 32 * t + c]);
            mg[t] = gld(&a.mg[l0 + 32 * t + c]);
        }
    }
    __device__ __forceinline__ void prefetch(uint32_t gb, int h, int j) {
        lbv[j] = *(const PCV_GLOBAL f32x4*)(a.lb + (size_t)gb * 32 + 8 * j + 4 * h);
    }
    __device__ __forceinline__ void end(const float (&)[NT], int, int) {}
    __device__ __forceinline__ void block(const f32x16 (&acc)[NT], const float (&)[NT], const f32x4 (&rb)[4], const PairWhere& at) {
        const int c = at.c, h = at.h;
        // the row's bound: the largest certified lower end s - mg over the tile's labels, joined with what earlier tiles left
        float lo[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float rbi = rb[i >> 2][i & 3];
            float m = -__builtin_inff();
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float s = acc[t][i] * rbi * w[t];
                m = (rbi > 0.0f && w[t] > 0.0f) ? fmaxf(m, s - mg[t]) : m;
            }
            lo[i] = m;
        }
#pragma unroll
        for (int off = 1; off < 32; off <<= 1)
#pragma unroll
            for (int i = 0; i < 16; ++i) lo[i] = fmaxf(lo[i], __shfl_xor(lo[i], off));
#pragma unroll
        for (int i = 0; i < 16; ++i) lo[i] = fmaxf(lo[i], lbv[i >> 2][i & 3]);
        if (c == 0) {  // (this wave is the only one that has the block in this launch; launches follow each other on the stream)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 v = {lo[4 * j], lo[4 * j + 1], lo[4 * j + 2], lo[4 * j + 3]};
                *(PCV_GLOBAL f32x4*)(a.lb + (size_t)at.gb * 32 + 8 * j + 4 * h) = v;
            }
        }
        // a wild row or label: every defined pair (scan.h); otherwise the certified upper end against the bound
        auto passes = [&](int t, int i) -> bool {
            const float rbi = rb[i >> 2][i & 3];
            if (rbi == 0.0f || w[t] == 0.0f) return false;
            if (rbi < 0.0f || w[t] < 0.0f) return true;
            return acc[t][i] * rbi * w[t] + mg[t] >= lo[i];
        };
        uint32_t mask[NT];
        uint32_t n = 0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            mask[t] = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) mask[t] |= passes(t, i) ? (1u << i) : 0u;
            n += (uint32_t)__builtin_popcount(mask[t]);
        }
        if (n) {
            unsigned long long k = g_atomic_add64(&a.counters[0], n);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (mask[t] & (1u << i)) {
                        if (k < a.cand_cap) {
                            const float rbi = rb[i >> 2][i & 3];
                            const float s = (rbi < 0.0f || w[t] < 0.0f) ? __builtin_inff() : acc[t][i] * rbi * w[t];
                            gst(&a.cand[k], ((uint64_t)at.partner_row(i) << 32) | (l0 + 32u * t + (uint32_t)c));
                            gst(&a.cand_s[k], s);
                        }
                        ++k;
                    }
                }
            }
        }
    }
};

// grid: x = span of row blocks [x * span_blocks, + span_blocks), cut at the launch's end; wave w of the workgroup takes the blocks
// first + w, first + w + kScreenWaves, ...  The label tile is a.tile, already in the swizzled bf16 order of the LDS tile (lab_tile).
// D[row of the streamed block][label of the tile] (pair_screen.h, with labels where it has tile rows) — the reduction over the labels
// of a row is over t in the lane and over the 32 lanes of a half.
template <int NT>
__global__ __launch_bounds__(kScreenWaves * 64) void assign_screen_kernel(const ScanParams* __restrict__ pp, const AssignArgs a) {
    const ScanParams& p = *pp;
    extern __shared__ uint4 lq[];  // [NT*32][Dp/8] 16-byte pieces of 8 bf16, swizzled
    const int P8 = p.D4 >> 1;
    const uint32_t TB = p.total_blocks;
    const uint64_t first = (uint64_t)blockIdx.x * a.span_blocks;
    if (first >= TB) return;  // (the whole workgroup)
    const uint32_t b0 = (uint32_t)first;
    const uint32_t b1 = (uint32_t)min((uint64_t)TB, first + a.span_blocks);

    {
        const u32x4* src = (const u32x4*)(a.lab_tile + (size_t)a.tile * NT * 32 * P8);
        for (int i = threadIdx.x; i < NT * 32 * P8; i += kScreenWaves * 64) lq[i] = __builtin_bit_cast(uint4, *(const PCV_GLOBAL u32x4*)(src + i));
    }
    __syncthreads();

    const uint32_t wave = uniform(threadIdx.x >> 6);
    if (b0 + wave >= b1) return;
    AssignPolicy<NT> pol{a};
    pair_stream<NT, false>(p, lq, a.rinv, 0, b0 + wave, b1, kScreenWaves, pol);
}

// one thread per candidate: its canonical score if it passes the final bound, and the row's running maximum
__global__ __launch_bounds__(256) void assign_rescore_kernel(const ScanParams* __restrict__ pp, const AssignArgs a) {
    const ScanParams& p = *pp;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_cand) return;
    const uint64_t cd = gld(&a.cand[i]);
    const uint32_t lr = (uint32_t)(cd >> 32), j = (uint32_t)cd;
    unsigned long long key = 0;
    if (gld(&a.cand_s[i]) + gld(&a.mg[j]) >= gld(&a.lb[lr])) {
        const RowRef r = row_ref(p, lr);
        const float4* y[1] = {a.lab_blk + (size_t)(j >> 5) * p.D4 * 32 + (j & 31)};
        double acc[1];
        pair_sums<1>(r.x, y, p.D4, acc, 32);
        const double cc = finish_score(a.metric, acc[0], gld(&a.norm[lr]), gld(&a.lab_norm[j]));
        if (cc == cc) {
            key = f64_key(cc);
            g_atomic_max64(&a.best_key[lr], key);
        }
    }
    gst(&a.cand_key[i], key);
}

// ... and the lowest label among those that reach it
__global__ __launch_bounds__(256) void assign_pick_kernel(const AssignArgs a) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_cand) return;
    const unsigned long long key = gld(&a.cand_key[i]);
    if (key == 0) return;
    const uint64_t cd = gld(&a.cand[i]);
    const uint32_t lr = (uint32_t)(cd >> 32);
    if (key == gld(&a.best_key[lr])) g_atomic_min(&a.best_lab[lr], (uint32_t)cd);
}

// one thread per launch row: the outputs by position among the selected rows, the histogram, the rows that changed their label
__global__ __launch_bounds__(256) void assign_finish_kernel(const ScanParams* __restrict__ pp, const AssignArgs a) {
    const ScanParams& p = *pp;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)p.total_blocks * 32) return;
    const RowRef r = row_ref(p, (uint32_t)i);
    int32_t label = -1;
    if (r.row < gld(&r.sg->nrows)) {
        const unsigned long long key = gld(&a.best_key[i]);
        float score = __builtin_nanf("");
        if (key != 0) {
            label = (int32_t)gld(&a.best_lab[i]);
            score = reported_score(a.metric, p.D, key_f64(key));
            g_atomic_add_i64(&a.out_counts[label], 1ll);
        }
        const int64_t o = gld(&a.seg_out0[r.sg - p.seg]) + (int64_t)r.row;
        gst(&a.out_label[o], label);
        gst(&a.out_score[o], score);
        gst(&a.out_ids[o], row_id(r));
    }
    const unsigned long long moved = __ballot(gld(&a.row_label[i]) != label);  // (row_label starts at -1)
    if ((threadIdx.x & 63) == (unsigned)__builtin_ctzll(moved | (1ull << 63)) && moved) g_atomic_add64(&a.counters[1], (unsigned long long)__builtin_popcountll(moved));
    gst(&a.row_label[i], label);
}

// ---- top-m labels (pcv_searcher_assign_top; DESIGN.md §4 "Top-m labels") ----

__device__ __forceinline__ uint32_t g_atomic_add32(uint32_t* p, uint32_t v) {
    return __hip_atomic_fetch_add((PCV_GLOBAL uint32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The two epilogues of the top-m screen over one label tile; begin() is AssignPolicy's.
//   bound (LIST = false): the lane's maximum of s - mg over its NT labels — one column of the tile — for each of its 16 rows, stored
//         as it is: colmax[row][c].  A store instruction covers two rows of 128 contiguous bytes; no value crosses a lane.
//   list  (LIST = true):  thr is the row's final threshold (a.lb, loaded as AssignPolicy loads lb); every (row, label) with
//         s + mg >= thr, and every defined pair with a wild row or label, is appended as AssignPolicy appends.
template <int NT, bool LIST>
struct AssignTopPolicy {
    const AssignTopArgs& x;
    uint32_t l0;
    float w[NT], mg[NT];
    f32x4 thr[4];
    __device__ __forceinline__ void begin(uint32_t, int c) {
        l0 = x.a.tile * NT * 32;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            w[t] = gld(&x.a.w[l0 + 32 * t + c]);
            mg[t] = gld(&x.a.mg[l0 + 32 * t + c]);
        }
    }
    __device__ __forceinline__ void prefetch(uint32_t gb, int h, int j) {
        if constexpr (LIST) thr[j] = *(const PCV_GLOBAL f32x4*)(x.a.lb + (size_t)gb * 32 + 8 * j + 4 * h);
    }
    __device__ __forceinline__ void end(const float (&)[NT], int, int) {}
    __device__ __forceinline__ void block(const f32x16 (&acc)[NT], const float (&)[NT], const f32x4 (&rb)[4], const PairWhere& at) {
        const int c = at.c;
        if constexpr (!LIST) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float rbi = rb[i >> 2][i & 3];
                float m = -__builtin_inff();
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float s = acc[t][i] * rbi * w[t];
                    m = (rbi > 0.0f && w[t] > 0.0f) ? fmaxf(m, s - mg[t]) : m;
                }
                gst(&x.colmax[(size_t)at.partner_row(i) * 32 + c], m);
            }
        } else {
            auto passes = [&](int t, int i) -> bool {
                const float rbi = rb[i >> 2][i & 3];
                if (rbi == 0.0f || w[t] == 0.0f) return false;
                if (rbi < 0.0f || w[t] < 0.0f) return true;
                return acc[t][i] * rbi * w[t] + mg[t] >= thr[i >> 2][i & 3];
            };
            uint32_t mask[NT];
            uint32_t n = 0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                mask[t] = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) mask[t] |= passes(t, i) ? (1u << i) : 0u;
                n += (uint32_t)__builtin_popcount(mask[t]);
            }
            if (n) {
                unsigned long long k = g_atomic_add64(&x.a.counters[0], n);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        if (mask[t] & (1u << i)) {
                            if (k < x.a.cand_cap) {
                                const float rbi = rb[i >> 2][i & 3];
                                const float s = (rbi < 0.0f || w[t] < 0.0f) ? __builtin_inff() : acc[t][i] * rbi * w[t];
                                gst(&x.a.cand[k], ((uint64_t)at.partner_row(i) << 32) | (l0 + 32u * t + (uint32_t)c));
                                gst(&x.a.cand_s[k], s);
                            }
                            ++k;
                        }
                    }
                }
            }
        }
    }
};

// grid, tile and stream exactly as assign_screen_kernel
template <int NT, bool LIST>
__global__ __launch_bounds__(kScreenWaves * 64) void assign_top_screen_kernel(const ScanParams* __restrict__ pp, const AssignTopArgs x) {
    const ScanParams& p = *pp;
    extern __shared__ uint4 lq[];  // [NT*32][Dp/8] 16-byte pieces of 8 bf16, swizzled
    const int P8 = p.D4 >> 1;
    const uint32_t TB = p.total_blocks;
    const uint64_t first = (uint64_t)blockIdx.x * x.a.span_blocks;
    if (first >= TB) return;  // (the whole workgroup)
    const uint32_t b0 = (uint32_t)first;
    const uint32_t b1 = (uint32_t)min((uint64_t)TB, first + x.a.span_blocks);

    {
        const u32x4* src = (const u32x4*)(x.a.lab_tile + (size_t)x.a.tile * NT * 32 * P8);
        for (int i = threadIdx.x; i < NT * 32 * P8; i += kScreenWaves * 64) lq[i] = __builtin_bit_cast(uint4, *(const PCV_GLOBAL u32x4*)(src + i));
    }
    __syncthreads();

    const uint32_t wave = uniform(threadIdx.x >> 6);
    if (b0 + wave >= b1) return;
    AssignTopPolicy<NT, LIST> pol{x};
    pair_stream<NT, false>(p, lq, x.a.rinv, 0, b0 + wave, b1, kScreenWaves, pol);
}

// one thread per launch row: the tile's 32 column maxima go into the row's eight largest so far (tile 0 starts the list), kept
// descending by a compare-exchange chain over registers; the threshold the list pass tests against is rewritten behind every tile and
// final behind the last.  The m-th largest of maxima of disjoint label sets is at most the m-th largest s - mg: a valid bound, weaker.
__global__ __launch_bounds__(256) void assign_top_merge_kernel(const AssignTopArgs x, uint32_t launch_rows) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= launch_rows) return;
    float top[kMaxTopLabels];
    if (x.a.tile == 0) {
#pragma unroll
        for (int k = 0; k < kMaxTopLabels; ++k) top[k] = -__builtin_inff();
    } else {
#pragma unroll
        for (int q = 0; q < kMaxTopLabels / 4; ++q) {
            const f32x4 v = *(const PCV_GLOBAL f32x4*)(x.topm + (size_t)i * kMaxTopLabels + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) top[4 * q + e] = v[e];
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const f32x4 v = *(const PCV_GLOBAL f32x4*)(x.colmax + (size_t)i * 32 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float in = v[e];
#pragma unroll
            for (int k = 0; k < kMaxTopLabels; ++k) {
                const float hi = fmaxf(top[k], in);
                in = fminf(top[k], in);
                top[k] = hi;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kMaxTopLabels / 4; ++q) {
        const f32x4 v = {top[4 * q], top[4 * q + 1], top[4 * q + 2], top[4 * q + 3]};
        *(PCV_GLOBAL f32x4*)(x.topm + (size_t)i * kMaxTopLabels + 4 * q) = v;
    }
    float thr = -__builtin_inff();
    if (gld(&x.a.rinv[i]) > 0.0f) {
#pragma unroll
        for (int k = 0; k < kMaxTopLabels; ++k) thr = (k == x.m - 1) ? top[k] : thr;
        if (x.a.metric == PCV_METRIC_COSINE) thr = fmaxf(thr, __double2float_rd((double)x.min_score - (double)x.a.margin));
    }
    gst(&x.a.lb[i], thr);
}

// one thread per candidate (the list pass tested the final threshold: all of them): the canonical score, stored with the label in a
// slot of the row's stretch — the image 0 where c is undefined or below the call's bound, the f64 comparison the screen cannot make.
// row_cnt counts down: which slot a candidate gets depends on the order the atomics land in, what the select step reads does not.
__global__ __launch_bounds__(256) void assign_top_rescore_kernel(const ScanParams* __restrict__ pp, const AssignTopArgs x) {
    const ScanParams& p = *pp;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= x.a.n_cand) return;
    const uint64_t cd = gld(&x.a.cand[i]);
    const uint32_t lr = (uint32_t)(cd >> 32), j = (uint32_t)cd;
    const RowRef r = row_ref(p, lr);
    const float4* y[1] = {x.a.lab_blk + (size_t)(j >> 5) * p.D4 * 32 + (j & 31)};
    double acc[1];
    pair_sums<1>(r.x, y, p.D4, acc, 32);
    const double cc = finish_score(x.a.metric, acc[0], gld(&x.a.norm[lr]), gld(&x.a.lab_norm[j]));
    const uint32_t slot = gld(&x.row_off[lr]) + g_atomic_add32(&x.row_cnt[lr], 0xffffffffu) - 1u;
    gst(&x.sorted_key[slot], (cc == cc && cc >= (double)x.min_score) ? f64_key(cc) : 0ull);
    gst(&x.sorted_lab[slot], j);
}

// (key descending, label ascending): x comes before y
__device__ __forceinline__ bool label_before(unsigned long long kx, uint32_t lx, unsigned long long ky, uint32_t ly) {
    return kx > ky || (kx == ky && lx < ly);
}

// a wave per launch row.  A row's entries are distinct (a label is listed once per row), so "the best entry strictly behind the last
// pick" walks them in order without marking any (neighbors_select_kernel); the outputs go by position among the selected rows.
__global__ __launch_bounds__(256) void assign_top_select_kernel(const ScanParams* __restrict__ pp, const AssignTopArgs x) {
    const ScanParams& p = *pp;
    const uint32_t lr = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (lr >= p.total_blocks * 32) return;  // (the whole wave)
    const int lane = threadIdx.x & 63;
    const RowRef r = row_ref(p, lr);
    if (r.row >= gld(&r.sg->nrows)) return;
    const int64_t o = gld(&x.a.seg_out0[r.sg - p.seg]) + (int64_t)r.row;
    const uint32_t e0 = gld(&x.row_off[lr]), e1 = gld(&x.row_off[lr + 1]);
    unsigned long long last_key = ~0ull;  // (no image is all ones: that would be a NaN)
    uint32_t last_lab = 0;
    int n = 0;
    for (; n < x.m; ++n) {
        unsigned long long bk = 0;
        uint32_t bl = 0xffffffffu;
        for (uint32_t e = e0 + lane; e < e1; e += 64) {
            const unsigned long long key = gld(&x.sorted_key[e]);
            const uint32_t lab = gld(&x.sorted_lab[e]);
            if (key != 0 && label_before(last_key, last_lab, key, lab) && label_before(key, lab, bk, bl)) {
                bk = key;
                bl = lab;
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long ok = shfl_xor_u64(bk, off);
            const uint32_t ol = __shfl_xor(bl, off);
            if (label_before(ok, ol, bk, bl)) {
                bk = ok;
                bl = ol;
            }
        }
        if (bk == 0) break;  // (wave-uniform after the exchange)
        last_key = bk;
        last_lab = bl;
        if (lane == 0) {
            gst(&x.out_labels[o * x.m + n], (int32_t)bl);
            gst(&x.out_scores[o * x.m + n], reported_score(x.a.metric, p.D, key_f64(bk)));
            g_atomic_add_i64(&x.out_label_rows[bl], 1ll);
        }
    }
    for (int j = n + lane; j < x.m; j += 64) {
        gst(&x.out_labels[o * x.m + j], (int32_t)-1);
        gst(&x.out_scores[o * x.m + j], __builtin_nanf(""));
    }
    if (lane == 0) {
        gst(&x.a.out_ids[o], row_id(r));
        gst(&x.out_count[o], (int32_t)n);
    }
}

constexpr int kSumBlocks = 8;  // row blocks of one label_sums workgroup

// grid: x = kSumBlocks row blocks; thread = one 16-byte piece of four features (pieces tid, tid + 256, ...).  The rows are walked in
// order and a run of rows with one label is summed in registers before it goes to S: fewer atomics where neighbours share a label,
// the same bits either way.
__global__ __launch_bounds__(256) void label_sums_kernel(const ScanParams* __restrict__ pp, const AssignArgs a) {
    const ScanParams& p = *pp;
    const int D4 = p.D4, Dp = D4 * 4;
    const uint32_t gb0 = blockIdx.x * kSumBlocks, gb1 = min(p.total_blocks, gb0 + kSumBlocks);
    for (int f = threadIdx.x; f < D4; f += 256) {
        long long s0 = 0, s1 = 0, s2 = 0, s3 = 0, members = 0;
        int cur = -1;
        auto flush = [&]() {
            if (cur >= 0) {
                if (f == 0) g_atomic_add_i64(&a.sum_counts[cur], members);
                long long* d = a.sums + (size_t)cur * Dp + 4 * f;
                if (s0) g_atomic_add_i64(d, s0);
                if (s1) g_atomic_add_i64(d + 1, s1);
                if (s2) g_atomic_add_i64(d + 2, s2);
                if (s3) g_atomic_add_i64(d + 3, s3);
            }
            s0 = s1 = s2 = s3 = members = 0;
        };
        int si = -1;
        for (uint32_t gb = gb0; gb < gb1; ++gb) {
            si = find_seg(p, gb, si < 0 ? 0 : si);
            const SegDesc* sg = &p.seg[si];
            const float4* blk = gld(&sg->blk) + ((size_t)(gb - gld(&sg->blk0)) * D4 + f) * 32;
            for (int r = 0; r < 32; ++r) {
                const size_t lr = (size_t)gb * 32 + r;
                const int lab = gld(&a.row_label[lr]);
                if (lab < 0 || lab >= a.K) continue;
                const double n = gld(&a.norm[lr]);
                if (!has_cosine(n)) continue;  // the row adds nothing
                if (lab != cur) {
                    flush();
                    cur = lab;
                }
                const double rs = unit_scale(n);
                const float4 v = gld4(blk + r);
                s0 += unit_int(v.x, rs);
                s1 += unit_int(v.y, rs);
                s2 += unit_int(v.z, rs);
                s3 += unit_int(v.w, rs);
                ++members;
            }
        }
        flush();
    }
}

}  // namespace

void launch_assign_labels(hipStream_t st, const ScanParams& p, const AssignArgs& a) {
    assign_labels_kernel<<<cdiv64((int64_t)a.label_blocks * 32 * (p.D4 / 2), 256), 256, 0, st>>>(a, p.D4);
    PCV_LAUNCHED();
}

void launch_assign_begin(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignArgs& a) {
    if (p.total_blocks == 0) return;
    assign_begin_kernel<<<cdiv64((int64_t)p.total_blocks * 32, 256), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

void launch_assign_screen(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t NT = a.tile_blocks;
    PCV_REQUIRE((NT == 1 || NT == 2 || NT == 4) && a.span_blocks >= 1 && (a.tile + 1) * NT <= a.label_blocks,
                "assign screen: bad tile (%u blocks, tile %u of %u label blocks, spans of %u)", NT, a.tile, a.label_blocks, a.span_blocks);
    const size_t lds = (size_t)NT * 32 * p.D4 * 4 * sizeof(uint16_t);
    const unsigned grid = (p.total_blocks + a.span_blocks - 1) / a.span_blocks;
#define PCV_ASSIGN(N)                                                    \
    allow_dynamic_lds((const void*)assign_screen_kernel<N>, lds);        \
    assign_screen_kernel<N><<<grid, kScreenWaves * 64, lds, st>>>(dp, a);
    if (NT == 4) {
        PCV_ASSIGN(4)
    } else if (NT == 2) {
        PCV_ASSIGN(2)
    } else {
        PCV_ASSIGN(1)
    }
#undef PCV_ASSIGN
    PCV_LAUNCHED();
}

void launch_assign_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignArgs& a) {
    if (a.n_cand == 0) return;
    assign_rescore_kernel<<<cdiv64((int64_t)a.n_cand, 256), 256, 0, st>>>(dp, a);
    assign_pick_kernel<<<cdiv64((int64_t)a.n_cand, 256), 256, 0, st>>>(a);
    PCV_LAUNCHED();
}

void launch_assign_finish(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignArgs& a) {
    if (p.total_blocks == 0) return;
    assign_finish_kernel<<<cdiv64((int64_t)p.total_blocks * 32, 256), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

namespace {
template <bool LIST>
void launch_top_screen(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignTopArgs& x) {
    if (p.total_blocks == 0) return;
    const AssignArgs& a = x.a;
    const uint32_t NT = a.tile_blocks;
    PCV_REQUIRE((NT == 1 || NT == 2 || NT == 4) && a.span_blocks >= 1 && (a.tile + 1) * NT <= a.label_blocks,
                "assign_top screen: bad tile (%u blocks, tile %u of %u label blocks, spans of %u)", NT, a.tile, a.label_blocks, a.span_blocks);
    const size_t lds = (size_t)NT * 32 * p.D4 * 4 * sizeof(uint16_t);
    const unsigned grid = (p.total_blocks + a.span_blocks - 1) / a.span_blocks;
#define PCV_ASSIGN_TOP(N)                                                          \
    allow_dynamic_lds((const void*)assign_top_screen_kernel<N, LIST>, lds);        \
    assign_top_screen_kernel<N, LIST><<<grid, kScreenWaves * 64, lds, st>>>(dp, x);
    if (NT == 4) {
        PCV_ASSIGN_TOP(4)
    } else if (NT == 2) {
        PCV_ASSIGN_TOP(2)
    } else {
        PCV_ASSIGN_TOP(1)
    }
#undef PCV_ASSIGN_TOP
    PCV_LAUNCHED();
}
}  // namespace

void launch_assign_top_bound(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignTopArgs& x) { launch_top_screen<false>(st, p, dp, x); }

void launch_assign_top_list(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignTopArgs& x) { launch_top_screen<true>(st, p, dp, x); }

void launch_assign_top_merge(hipStream_t st, const ScanParams& p, const AssignTopArgs& x) {
    if (p.total_blocks == 0) return;
    PCV_REQUIRE(x.m >= 1 && x.m <= kMaxTopLabels, "assign_top merge: m = %d", x.m);
    assign_top_merge_kernel<<<cdiv64((int64_t)p.total_blocks * 32, 256), 256, 0, st>>>(x, p.total_blocks * 32);
    PCV_LAUNCHED();
}

void launch_assign_top_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignTopArgs& x) {
    if (p.total_blocks == 0) return;
    launch_owner_offsets(st, x.a.cand, x.a.n_cand, x.row_cnt, x.row_off, p.total_blocks * 32);
    if (x.a.n_cand) assign_top_rescore_kernel<<<cdiv64((int64_t)x.a.n_cand, 256), 256, 0, st>>>(dp, x);
    PCV_LAUNCHED();
}

void launch_assign_top_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignTopArgs& x) {
    if (p.total_blocks == 0) return;
    assign_top_select_kernel<<<cdiv64((int64_t)p.total_blocks * 32, 4), 256, 0, st>>>(dp, x);
    PCV_LAUNCHED();
}

void launch_label_sums(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignArgs& a) {
    if (p.total_blocks == 0) return;
    label_sums_kernel<<<(p.total_blocks + kSumBlocks - 1) / kSumBlocks, 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

}  // namespace pcv
