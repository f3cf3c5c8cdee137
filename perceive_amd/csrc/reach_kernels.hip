// reach_kernels.hip — the device steps of pcv_searcher_reach_tree (DESIGN.md §4 "Reach tree") that the linkage tree does not have:
// the spanning tree of the participating rows under the mutual-reachability weight w(a, b) = min(core(a), core(b), c(a, b)), exact, in
// the Borůvka rounds of linkage_kernels.hip with the cap applied.  The norms come from selfjoin_prep_kernel, the candidates of the
// core step from the neighbours' bound, threshold, list and rescore (neighbors_kernels.hip) with k = j; begin, cert, threshold, merge,
// flatten and settle are the linkage kernels themselves (launch_linkage_*), which see the LinkageArgs inside ReachArgs.  Here:
//
//   reach_core_kernel                   a wave per launch row: the j-th largest f64 image among the row's rescored candidates, found
//                                       bit by bit from the top -> core[launch row]
//   reach_images_kernel                 klo = core rounded down to f32, khi = core rounded up (both +inf for j == 0, -inf for a row
//                                       that takes no part, whose core is NaN)
//   reach_screen_kernel<NT, false>      the bound pass: linkage_screen_kernel's (a further copy of its staging and MFMA loop: that
//                                       kernel's code object must not move), raising min(s, klo[a], klo[b]) instead of s
//   reach_screen_kernel<NT, true>       the list pass: (owner a, partner b) is a candidate iff both take part, s >= thr[comp[a]] (or
//                                       a row is wild), comp[a] != comp[b], khi[a] >= thr and khi[b] >= thr.  The owner's core test
//                                       is folded into its threshold when the tile is staged (+inf when it fails); the partner's khi
//                                       is loaded on demand inside the rare branch, next to its component
//   reach_rescore_kernel, _choose       c as linkage_rescore_kernel computes it, w = min(core[a], core[b], c) in f64, the 64-bit
//                                       atomic max of f64_key(w), then the 64-bit atomic min of the pair among those that reach it
//   reach_rows_kernel, _edges           the outputs by position; an edge's c is computed once more
#include "device_access.h"
#include "launch_rows.h"
#include "row_jobs.h"

namespace pcv {
namespace {

constexpr int kReachWaves = 8;  // waves of a screen workgroup (kLinkWaves)

__device__ __forceinline__ void g_atomic_max64(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_max((PCV_GLOBAL unsigned long long*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void g_atomic_min64(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_min((PCV_GLOBAL unsigned long long*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a wave per launch row.  The row's stretch of sorted_key holds the image of c with every partner the neighbours' list pass left it:
// all of its j best are among them.  The largest T with at least j images >= T is the j-th largest image, ties counted as often as
// they occur.  A participating row with fewer than j images is counted in *short_rows (for the host, an internal error).
__global__ __launch_bounds__(256) void reach_core_kernel(const ReachArgs a, uint32_t launch_rows) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= launch_rows) return;  // (the whole wave)
    const int lane = threadIdx.x & 63;
    if (gld(&a.l.rinv[row]) == 0.0f) {
        if (lane == 0) gst(&a.core[row], (double)__builtin_nanf(""));
        return;
    }
    const uint32_t e0 = gld(&a.row_off[row]), e1 = gld(&a.row_off[row + 1]);
    unsigned long long T = 0;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long cand = T | (1ull << bit);
        int n = 0;
        for (uint32_t e = e0; e < e1; e += 64) {  // (wave-uniform bounds: the whole wave votes)
            const uint32_t i = e + (uint32_t)lane;
            const unsigned long long key = i < e1 ? gld(&a.sorted_key[i]) : 0ull;
            n += __builtin_popcountll(__ballot(key >= cand));
        }
        if (n >= a.k) T = cand;
    }
    if (lane != 0) return;
    if (T == 0) {
        (void)g_atomic_add64(a.short_rows, 1ull);
        gst(&a.core[row], (double)__builtin_nanf(""));
    } else {
        gst(&a.core[row], key_f64(T));
    }
}

// one thread per launch row.  have_core == 0 (j == 0): core = +inf for the rows that take part, NaN for the others
__global__ __launch_bounds__(256) void reach_images_kernel(const ReachArgs a, uint32_t launch_rows, int have_core) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= launch_rows) return;
    const bool part = gld(&a.l.rinv[i]) != 0.0f;
    double core;
    if (have_core) {
        core = gld(&a.core[i]);
    } else {
        core = part ? (double)__builtin_inff() : (double)__builtin_nanf("");
        gst(&a.core[i], core);
    }
    const bool ok = part && core == core;
    gst(&a.klo[i], ok ? __double2float_rd(core) : -__builtin_inff());
    gst(&a.khi[i], ok ? __double2float_ru(core) : -__builtin_inff());
}

// linkage_cert_kernel: cert[root] = 1 where the component has a certified row
__global__ __launch_bounds__(256) void reach_cert_kernel(const ReachArgs a, uint32_t launch_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= launch_rows) return;
    if (gld(&a.l.rinv[i]) > 0.0f) (void)g_atomic_max(&a.l.cert[gld(&a.l.comp[i])], 1u);
}

// grid, tile, stream and accumulator layout: linkage_screen_kernel, to the letter.  What differs is marked "the cap".
template <int NT, bool LIST>
__global__ __launch_bounds__(kReachWaves * 64) void reach_screen_kernel(const ScanParams* __restrict__ pp, const ReachArgs ra_) {
    const ScanParams& p = *pp;
    const LinkageArgs& a = ra_.l;
    extern __shared__ uint4 lq[];  // [NT*32][Dp/8] 16-byte pieces of 8 bf16, swizzled
    __shared__ const float4* tbase[NT];
    const int D4 = p.D4, P8 = D4 >> 1, NCH = D4 >> 4;
    const uint32_t TB = p.total_blocks;
    const uint32_t tb0 = blockIdx.x * NT;
    const uint32_t step = kReachWaves * a.stride;  // launch blocks between two blocks of a wave
    const uint32_t SB = (TB + a.stride - 1) / a.stride;
    const uint64_t first = (uint64_t)blockIdx.y * a.walk_len;
    if (first >= SB) return;  // (the whole workgroup)
    const uint32_t b0 = (uint32_t)first * a.stride;
    const uint32_t b1 = (uint32_t)min((uint64_t)SB, first + a.walk_len) * a.stride;  // every sampled block below it is below TB

    if (threadIdx.x < NT) {
        const uint32_t gb = tb0 + threadIdx.x;
        const float4* base = nullptr;
        if (gb < TB) {
            const SegDesc& sg = p.seg[find_seg(p, gb)];
            base = gld(&sg.blk) + (size_t)(gb - gld(&sg.blk0)) * D4 * 32;
        }
        tbase[threadIdx.x] = base;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NT * 32 * P8; i += kReachWaves * 64) {
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

    const int lane = threadIdx.x & 63;
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    if (b0 + wave * a.stride >= b1) return;  // (no workgroup barrier behind this point)
    // ra, bd, ca: linkage_screen_kernel.  The cap: the list pass's bd is +inf where the owner's khi is below its component's
    // threshold (no edge of the owner can be the component's best); ka is the bound pass's klo of each tile row
    float ra[NT], bd[NT];
    uint32_t ca[LIST ? 1 : NT];
    float ka[LIST ? 1 : NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const size_t row = (size_t)(tb0 + t) * 32 + c;
        ra[t] = gld(&a.rinv[row]);
        const uint32_t cr = gld(&a.comp[row]);
        if (LIST) {
            const float th = gld(&a.thr[cr]);
            bd[t] = gld(&ra_.khi[row]) >= th ? th : __builtin_inff();
        } else {
            bd[t] = -__builtin_inff();
            ca[t] = cr;
            ka[t] = gld(&ra_.klo[row]);
        }
    }

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
    enter_block(cons, b0 + wave * a.stride);
    prod = cons;

    float4 buf[2][8];
    // (always issues its loads: past the end of the wave's stream they read a chunk of its last block again — scan_mfma_kernel)
    auto produce = [&](float4 (&b)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) b[i] = ld_piece<false>(prod.rows, lane_off + (uint32_t)((i >> 1) * 4 + (i & 1)) * 512u, (uint32_t)prod.ch * 8192u);
        if (prod.gb < b1 && ++prod.ch == NCH) enter_block(prod, prod.gb + step);
    };

    f32x4 rb[4];  // rinv of the block's rows 8 j + 4 h + (0..3): accumulators 4 j + (0..3)
    u32x4 cb[LIST ? 1 : 4];  // the bound pass: their components
    f32x4 kb[LIST ? 1 : 4];  // the cap, the bound pass: their klo
    auto rb_prefetch = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            rb[j] = *(const PCV_GLOBAL f32x4*)(a.rinv + (size_t)cons.gb * 32 + 8 * j + 4 * h);
            if (!LIST) {
                cb[j] = *(const PCV_GLOBAL u32x4*)(a.comp + (size_t)cons.gb * 32 + 8 * j + 4 * h);
                kb[j] = *(const PCV_GLOBAL f32x4*)(ra_.klo + (size_t)cons.gb * 32 + 8 * j + 4 * h);
            }
        }
    };
    auto owner_row = [&](int t) { return (tb0 + t) * 32u + (uint32_t)c; };
    auto partner_row = [&](int i) { return cons.gb * 32u + (uint32_t)((i & 3) + 8 * (i >> 2) + 4 * h); };

    // the list pass: (owner 32 t + c of the tile, partner i of the block) passes the score test
    auto passes = [&](int t, int i) -> bool {
        const float rbi = rb[i >> 2][i & 3];
        const float s = acc[t][i] * ra[t] * rbi;
        return (ra[t] > 0.0f && rbi > 0.0f) ? s >= bd[t] : (ra[t] != 0.0f && rbi != 0.0f);  // (a wild row: every pair, scan.h)
    };
    // the cap, the rare branch: the partner is of another component and its khi reaches the owner's threshold (bd is +inf for an
    // owner that failed its own test: no finite khi reaches that, and with j == 0 no owner fails)
    auto foreign = [&](int t, int i, uint32_t co) -> bool {
        const uint32_t pr = partner_row(i);
        return gld(&a.comp[pr]) != co && gld(&ra_.khi[pr]) >= bd[t];
    };

    auto epilogue = [&]() {
        if (NCH < 2) rb_prefetch();
        if (LIST) {
            uint32_t n = 0;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) n += passes(t, i) ? 1u : 0u;
            if (n) {
                uint32_t nf = 0;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const uint32_t co = gld(&a.comp[owner_row(t)]);
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        if (passes(t, i)) nf += foreign(t, i, co) ? 1u : 0u;
                }
                if (nf) {
                    unsigned long long at = g_atomic_add64(&a.counters[kLinkListed], nf);
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const uint32_t co = gld(&a.comp[owner_row(t)]);
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            if (passes(t, i) && foreign(t, i, co)) {
                                if (at < a.cand_cap) gst(&a.cand[at], ((uint64_t)owner_row(t) << 32) | partner_row(i));
                                ++at;
                            }
                        }
                    }
                }
            }
        } else {
            // the cap: the running maximum of min(s, klo of the owner, klo of the partner) over the certified rows of other components
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float m = bd[t];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float rbi = rb[i >> 2][i & 3];
                    const float s = fminf(acc[t][i] * ra[t] * rbi, fminf(ka[t], kb[i >> 2][i & 3]));
                    const bool ok = rbi > 0.0f && cb[i >> 2][i & 3] != ca[t];
                    m = ok ? fmaxf(m, s) : m;
                }
                bd[t] = m;
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
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
            epilogue();
            enter_block(cons, cons.gb + step);
        }
    };

    // one chunk of loads in flight while one feeds the matrix cores (every buf[] index a literal, or the array moves to scratch)
#define PCV_REACH_STEP(REFILL, CONS)                     \
    if (NCH >= 2 && cons.ch == NCH - 2) rb_prefetch();   \
    produce(buf[REFILL]);                                \
    consume(buf[CONS]);                                  \
    if (cons.gb >= b1) break;
    produce(buf[0]);
    while (true) {
        PCV_REACH_STEP(1, 0)
        PCV_REACH_STEP(0, 1)
    }
#undef PCV_REACH_STEP
    if (!LIST) {
        // publish (linkage_screen_kernel): max commutes, a lane whose maximum the word already holds leaves the atomic out
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float m = fmaxf(bd[t], __shfl_xor(bd[t], 32));
            if (h == 0 && ra[t] > 0.0f && m > -__builtin_inff()) {
                const uint32_t key = f32_key(m);
                if (ld_relaxed(&a.comp_max[ca[t]]) < key) (void)g_atomic_max(&a.comp_max[ca[t]], key);
            }
        }
    }
}

// one thread per candidate: the canonical cosine (linkage_rescore_kernel's arithmetic), capped by the two cores; the image of w is
// kept for the choose step and raised into the owner's component
__global__ __launch_bounds__(256) void reach_rescore_kernel(const ScanParams* __restrict__ pp, const ReachArgs ra_) {
    const ScanParams& p = *pp;
    const LinkageArgs& a = ra_.l;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_cand) return;
    const uint64_t cd = gld(&a.cand[i]);
    const uint32_t la = (uint32_t)(cd >> 32), lb = (uint32_t)cd;
    const RowRef ra = row_ref(p, la), rb = row_ref(p, lb);
    const float4* y[1] = {rb.x};
    double acc[1];
    pair_sums<1>(ra.x, y, p.D4, acc, 32);
    const double cc = finish_score(PCV_METRIC_COSINE, acc[0], gld(&a.norm[la]), gld(&a.norm[lb]));
    const double ka = gld(&ra_.core[la]), kb = gld(&ra_.core[lb]);
    double w = cc;
    w = ka < w ? ka : w;
    w = kb < w ? kb : w;
    const unsigned long long key = (cc == cc && ka == ka && kb == kb) ? f64_key(w) : 0ull;  // (both rows take part: all three are numbers)
    gst(&a.cand_key[i], key);
    if (key) g_atomic_max64(&a.best_key[gld(&a.comp[la])], key);
}

// linkage_choose_kernel, word for word: among the candidates that reach their component's best w, the lowest (lower row, higher row)
__global__ __launch_bounds__(256) void reach_choose_kernel(const ReachArgs ra_) {
    const LinkageArgs& a = ra_.l;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_cand) return;
    const unsigned long long key = gld(&a.cand_key[i]);
    const uint64_t cd = gld(&a.cand[i]);
    const uint32_t la = (uint32_t)(cd >> 32), lb = (uint32_t)cd;
    const uint32_t root = gld(&a.comp[la]);
    if (key == 0 || key != gld(&a.best_key[root])) return;
    const uint32_t lo = la < lb ? la : lb, hi = la < lb ? lb : la;
    g_atomic_min64(&a.best_pair[root], ((unsigned long long)lo << 32) | hi);
}

__device__ __forceinline__ int64_t reach_id(const RowRef& q) {
    const int64_t* ids = gld(&q.sg->ids);
    return ids ? gld(&ids[q.row]) : gld(&q.sg->id0) + (int64_t)q.row;
}

__global__ __launch_bounds__(256) void reach_rows_kernel(const ScanParams* __restrict__ pp, const ReachArgs ra_) {
    const ScanParams& p = *pp;
    const LinkageArgs& a = ra_.l;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)p.total_blocks * 32) return;
    const RowRef r = row_ref(p, (uint32_t)i);
    if (r.row >= gld(&r.sg->nrows)) return;
    const int64_t o = gld(&a.seg_out0[r.sg - p.seg]) + (int64_t)r.row;
    gst(&a.out_ids[o], reach_id(r));
    gst(&a.out_part[o], (int8_t)(gld(&a.rinv[i]) != 0.0f ? 1 : 0));
    gst(&ra_.out_core[o], gld(&ra_.core[i]));
}

__global__ __launch_bounds__(256) void reach_edges_kernel(const ScanParams* __restrict__ pp, const ReachArgs ra_) {
    const ScanParams& p = *pp;
    const LinkageArgs& a = ra_.l;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_edges) return;
    const unsigned long long pair = gld(&a.edge_pair[i]);
    const uint32_t la = (uint32_t)(pair >> 32), lb = (uint32_t)pair;
    const RowRef ra = row_ref(p, la), rb = row_ref(p, lb);
    const float4* y[1] = {rb.x};
    double acc[1];
    pair_sums<1>(ra.x, y, p.D4, acc, 32);
    PCV_GLOBAL ReachEdge* out = (PCV_GLOBAL ReachEdge*)&ra_.out_edges[i];
    out->w = key_f64(gld(&a.edge_key[i]));
    out->c = finish_score(PCV_METRIC_COSINE, acc[0], gld(&a.norm[la]), gld(&a.norm[lb]));
    out->pos_a = gld(&a.seg_out0[ra.sg - p.seg]) + (int64_t)ra.row;
    out->pos_b = gld(&a.seg_out0[rb.sg - p.seg]) + (int64_t)rb.row;
    out->id_a = reach_id(ra);
    out->id_b = reach_id(rb);
}

template <bool LIST>
void launch_screen(hipStream_t st, const ScanParams& p, const ScanParams* dp, const ReachArgs& ra) {
    if (p.total_blocks == 0) return;
    const LinkageArgs& a = ra.l;
    const uint32_t NT = a.tile_blocks;
    PCV_REQUIRE((NT == 1 || NT == 2 || NT == 4) && a.stride >= 1 && a.walk_len >= 1 && (!LIST || a.stride == 1),
                "reach screen: bad shape (tile of %u blocks, stride %u, walks of %u)", NT, a.stride, a.walk_len);
    const size_t lds = (size_t)NT * 32 * p.D4 * 4 * sizeof(uint16_t);
    const unsigned tiles = (p.total_blocks + NT - 1) / NT;
    const unsigned sampled = (p.total_blocks + a.stride - 1) / a.stride;
    const unsigned walks = (sampled + a.walk_len - 1) / a.walk_len;
    PCV_REQUIRE(walks <= 65535u, "reach screen: %u walks", walks);
    const dim3 grid(tiles, walks);
#define PCV_REACH(N)                                                          \
    allow_dynamic_lds((const void*)reach_screen_kernel<N, LIST>, lds);        \
    reach_screen_kernel<N, LIST><<<grid, kReachWaves * 64, lds, st>>>(dp, ra);
    if (NT == 4) {
        PCV_REACH(4)
    } else if (NT == 2) {
        PCV_REACH(2)
    } else {
        PCV_REACH(1)
    }
#undef PCV_REACH
    PCV_LAUNCHED();
}

}  // namespace

void launch_reach_core(hipStream_t st, const ScanParams& p, const ReachArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t launch_rows = p.total_blocks * 32;
    if (a.k >= 1) reach_core_kernel<<<cdiv64((int64_t)launch_rows, 4), 256, 0, st>>>(a, launch_rows);
    reach_images_kernel<<<cdiv64((int64_t)launch_rows, 256), 256, 0, st>>>(a, launch_rows, a.k >= 1 ? 1 : 0);
    PCV_LAUNCHED();
}

void launch_reach_bound(hipStream_t st, const ScanParams& p, const ScanParams* dp, const ReachArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t launch_rows = p.total_blocks * 32;
    reach_cert_kernel<<<cdiv64((int64_t)launch_rows, 256), 256, 0, st>>>(a, launch_rows);
    launch_screen<false>(st, p, dp, a);
}

void launch_reach_list(hipStream_t st, const ScanParams& p, const ScanParams* dp, const ReachArgs& a) { launch_screen<true>(st, p, dp, a); }

void launch_reach_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const ReachArgs& a) {
    if (a.l.n_cand == 0) return;
    reach_rescore_kernel<<<cdiv64((int64_t)a.l.n_cand, 256), 256, 0, st>>>(dp, a);
    reach_choose_kernel<<<cdiv64((int64_t)a.l.n_cand, 256), 256, 0, st>>>(a);
    PCV_LAUNCHED();
}

void launch_reach_output(hipStream_t st, const ScanParams& p, const ScanParams* dp, const ReachArgs& a) {
    if (p.total_blocks == 0) return;
    reach_rows_kernel<<<cdiv64((int64_t)p.total_blocks * 32, 256), 256, 0, st>>>(dp, a);
    if (a.l.n_edges) reach_edges_kernel<<<cdiv64((int64_t)a.l.n_edges, 256), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

}  // namespace pcv
