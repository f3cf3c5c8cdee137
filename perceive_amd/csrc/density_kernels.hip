// density_kernels.hip — the device steps of pcv_searcher_density_clusters (DESIGN.md §4 "Density clusters"): DBSCAN under the
// canonical cosine, exact, computed where the rows live.  The row prep (norms, rinv, the wild marking) is selfjoin_prep_kernel
// (launch_selfjoin_prep); then
//
//   1. density_screen_kernel<NT, false>  the degree pass: the tile-in-LDS, stream-the-blocks bf16 screen of selfjoin_screen_kernel (its
//                                        own copy of the staging and MFMA loop of pair_screen.h: see the kernel) with a
//                                        three-way epilogue.  s >= hi with both rows certified: a SURE pair, near whatever the f64
//                                        arithmetic would say — both rows' degrees go up and the pair is never listed.  lo <= s < hi,
//                                        or a wild row: a BAND pair, appended to one device list (overflow counted, one rerun by the
//                                        host, as for the duplicate pairs).  Below lo: not near.
//   2. density_rescore_kernel            one thread per band pair: the canonical f64 cosine (pair_sums and finish_score: the
//                                        arithmetic of selfjoin_rescore_kernel); c >= threshold raises both degrees and appends the
//                                        pair to the confirmed list.
//   3. density_core_kernel               one thread per launch row: core = takes part and degree + 1 >= min_items; parent = itself,
//                                        attach = none.
//   4. density_screen_kernel<NT, true>   the link pass: the same stream again, sure pairs only.  Two core rows: union.  One core
//                                        row: an atomic min of it into the other row's attach.  density_link_list_kernel does the
//                                        same for the confirmed band pairs.
//   5. density_flatten_kernel, density_rank_kernel, density_output_kernel
//                                        roots, their numbering by an exclusive prefix sum in launch-row (= global position) order,
//                                        labels, kinds, degrees, ids and the counters.
#include "device_access.h"
#include "launch_rows.h"
#include "pair_screen.h"
#include "row_jobs.h"

namespace pcv {
namespace {

constexpr uint32_t kNoRow = 0xffffffffu;

__device__ __forceinline__ uint32_t g_atomic_min32(uint32_t* p, uint32_t v) {
    return __hip_atomic_fetch_min((PCV_GLOBAL uint32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what a near pair of launch rows (la, lb) does to the forest: both core: one component; one core: it may be the other's cluster
__device__ __forceinline__ void density_link_pair(const DensityArgs& a, uint32_t la, uint32_t lb, bool core_a, bool core_b) {
    if (core_a && core_b)
        row_union(a.parent, la, lb);
    else if (core_a)
        (void)g_atomic_min32(&a.attach[lb], la);
    else if (core_b)
        (void)g_atomic_min32(&a.attach[la], lb);
}

// grid, tile, stream and accumulator layout: selfjoin_screen_kernel.  D[row of the streamed block][row of the tile]: lane
// (c = lane & 31, h = lane >> 5) holds tile rows 32 t + c and, in accumulator i, block row (i & 3) + 8 (i >> 2) + 4 h.
// LINK = false: the degree pass (degrees, sure-pair count, band list).  LINK = true: the link pass (sure pairs only -> parent, attach).
// The one screen that is NOT on the skeleton of pair_screen.h (DESIGN.md §4 "The row-pair screen"): ported to it (a DensityPolicy
// with dega, cam and wave_sure as members), no form had scratch and the registers fell (225 / 160 / 139 -> 223 / 157 / 135 and
// 221 / 166 / 147 -> 220 / 152 / 129), but at a million rows the degree pass took 1339 ms against 1284 (4.1 % slower) and the link
// pass 1128 against 1112 (1.5 %), outside the 0.5 % the old build's repeats span.  A fix to the stream in pair_screen.h has to be
// made here too.
template <int NT, bool LINK>
__global__ __launch_bounds__(kScreenWaves * 64) void density_screen_kernel(const ScanParams* __restrict__ pp, const DensityArgs a) {
    const ScanParams& p = *pp;
    extern __shared__ uint4 lq[];  // [NT*32][Dp/8] 16-byte pieces of 8 bf16, swizzled
    __shared__ const float4* tbase[NT];
    const int D4 = p.D4, P8 = D4 >> 1, NCH = D4 >> 4;
    const uint32_t TB = p.total_blocks;
    const uint32_t tb0 = blockIdx.x * NT;
    const uint64_t first = (uint64_t)tb0 + (uint64_t)blockIdx.y * a.span_blocks;
    if (first >= TB) return;  // (the whole workgroup)
    const uint32_t b0 = (uint32_t)first;
    const uint32_t b1 = (uint32_t)min((uint64_t)TB, first + a.span_blocks);

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

    const int lane = threadIdx.x & 63;
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    if (b0 + wave >= b1) return;
    float ra[NT];
    uint32_t cam = 0;  // LINK: bit t: the lane's row of tile block t is a core row
    // !LINK: sure partners of the lane's tile rows among the lane's block rows over the whole span, 16 bits a tile row: a lane meets
    // 16 rows of every eighth block of the span, 2 * span_blocks partners at most, and spans stay below 2^15 blocks (2^30 rows)
    uint32_t dega[(NT + 1) / 2];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        ra[t] = gld(&a.rinv[(size_t)(tb0 + t) * 32 + c]);  // (zero behind the launch's last block)
        if (LINK) cam |= gld(&a.core[(size_t)(tb0 + t) * 32 + c]) != 0 ? (1u << t) : 0u;
    }
#pragma unroll
    for (int t = 0; t < (NT + 1) / 2; ++t) dega[t] = 0;
    const float hi = a.hi, lo = a.lo;
    unsigned long long wave_sure = 0;  // (wave-uniform)

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
    enter_block(cons, b0 + wave);
    prod = cons;

    float4 buf[2][8];
    // (always issues its loads: past the end of the wave's stream they read a chunk of its last block again — scan_mfma_kernel)
    auto produce = [&](float4 (&b)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) b[i] = ld_piece<false>(prod.rows, lane_off + (uint32_t)((i >> 1) * 4 + (i & 1)) * 512u, (uint32_t)prod.ch * 8192u);
        if (prod.gb < b1 && ++prod.ch == NCH) enter_block(prod, prod.gb + kScreenWaves);
    };

    f32x4 rb[4];  // rinv of the block's rows 8 j + 4 h + (0..3): accumulators 4 j + (0..3)
    auto rb_prefetch = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) rb[j] = *(const PCV_GLOBAL f32x4*)(a.rinv + (size_t)cons.gb * 32 + 8 * j + 4 * h);
    };

    // 2: a sure pair, 1: a band pair, 0: not near (or, in a block of the tile's own, not row a before row b)
    auto classify = [&](int t, int i, bool diagonal) -> int {
        const float rbi = rb[i >> 2][i & 3];
        const float s = acc[t][i] * ra[t] * rbi;
        int k;
        if (ra[t] > 0.0f && rbi > 0.0f)
            k = s >= hi ? 2 : (s >= lo ? 1 : 0);
        else
            k = (ra[t] != 0.0f && rbi != 0.0f) ? 1 : 0;  // (a wild row: every pair is a band pair, scan.h)
        // row a before row b: (tb0 + t) * 32 + c < gb * 32 + (i & 3) + 8 (i >> 2) + 4 h, with the lane's part on one side and a
        // wave-uniform number on the other (tb0 <= gb < tb0 + NT here), so that nothing per accumulator is kept in registers
        if (diagonal && !(c - 4 * h < (i & 3) + 8 * (i >> 2) + (int)(cons.gb - tb0) * 32 - 32 * t)) k = 0;
        return k;
    };

    auto epilogue = [&]() {
        if (NCH < 2) rb_prefetch();
        const bool diagonal = cons.gb < tb0 + NT;  // the block is one of the tile's own: row a before row b only
        bool any = false;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) any |= classify(t, i, diagonal) >= (LINK ? 2 : 1);
        if (__any(any)) {
            if (LINK) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    uint32_t m = 0;
#pragma unroll
                    for (int i = 0; i < 16; ++i) m |= classify(t, i, diagonal) == 2 ? (1u << i) : 0u;
                    while (m) {
                        const int i = __builtin_ctz(m);
                        m &= m - 1;
                        const uint32_t lb = cons.gb * 32u + (uint32_t)((i & 3) + 8 * (i >> 2) + 4 * h);
                        density_link_pair(a, (tb0 + t) * 32u + (uint32_t)c, lb, (cam >> t) & 1u, gld(&a.core[lb]) != 0);
                    }
                }
            } else {
                // the streamed rows' side of the degrees: accumulator i is one block row per half-wave; its sure partners are
                // counted over the 32 lanes of the half and the tiles (both counts are wave-uniform), and the first lane of each
                // half adds them: one atomic per block row that has any
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    uint32_t n0 = 0, n1 = 0;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const bool sure = classify(t, i, diagonal) == 2;
                        dega[t >> 1] += sure ? (1u << (16 * (t & 1))) : 0u;
                        const unsigned long long bal = __ballot(sure);
                        n0 += (uint32_t)__builtin_popcount((uint32_t)bal);
                        n1 += (uint32_t)__builtin_popcount((uint32_t)(bal >> 32));
                    }
                    if (n0 + n1) {
                        const uint32_t mine = h ? n1 : n0;
                        if (c == 0 && mine) (void)g_atomic_add(&a.degree[cons.gb * 32u + (uint32_t)((i & 3) + 8 * (i >> 2) + 4 * h)], mine);
                        wave_sure += n0 + n1;
                    }
                }
                // the band pairs, listed as selfjoin_screen_kernel lists its candidates
                uint32_t mask[NT];
                uint32_t n = 0;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    mask[t] = 0;
#pragma unroll
                    for (int i = 0; i < 16; ++i) mask[t] |= classify(t, i, diagonal) == 1 ? (1u << i) : 0u;
                    n += (uint32_t)__builtin_popcount(mask[t]);
                }
                if (n) {
                    unsigned long long at = g_atomic_add64(&a.counters[kDensityBand], n);
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        uint32_t m = mask[t];
                        while (m) {
                            const int i = __builtin_ctz(m);
                            m &= m - 1;
                            if (at < a.cand_cap)
                                gst(&a.cand[at], ((uint64_t)((tb0 + t) * 32u + (uint32_t)c) << 32) | (cons.gb * 32u + (uint32_t)((i & 3) + 8 * (i >> 2) + 4 * h)));
                            ++at;
                        }
                    }
                }
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
            enter_block(cons, cons.gb + kScreenWaves);
        }
    };

    // one chunk of loads in flight while one feeds the matrix cores (every buf[] index a literal, or the array moves to scratch);
    // the block's rinv values are requested one chunk ahead of the epilogue and before that step's row loads
#define PCV_DENSITY_STEP(REFILL, CONS)                   \
    if (NCH >= 2 && cons.ch == NCH - 2) rb_prefetch();   \
    produce(buf[REFILL]);                                \
    consume(buf[CONS]);                                  \
    if (cons.gb >= b1) break;
    produce(buf[0]);
    while (true) {
        PCV_DENSITY_STEP(1, 0)
        PCV_DENSITY_STEP(0, 1)
    }
#undef PCV_DENSITY_STEP
    if (!LINK) {
        // the tile rows' side of the degrees: one atomic per lane and tile row for the whole span; the sure pairs: one per wave
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const uint32_t d = (dega[t >> 1] >> (16 * (t & 1))) & 0xffffu;
            if (d) (void)g_atomic_add(&a.degree[(size_t)(tb0 + t) * 32 + c], d);
        }
        if (lane == 0 && wave_sure) (void)g_atomic_add64(&a.counters[kDensitySure], wave_sure);
    }
}

__global__ __launch_bounds__(256) void density_rescore_kernel(const ScanParams* __restrict__ pp, const DensityArgs a) {
    const ScanParams& p = *pp;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_cand) return;
    const uint64_t cd = gld(&a.cand[i]);
    const uint32_t la = (uint32_t)(cd >> 32), lb = (uint32_t)cd;
    const RowRef ra = row_ref(p, la), rb = row_ref(p, lb);
    const float4* y[1] = {rb.x};
    double acc[1];
    pair_sums<1>(ra.x, y, p.D4, acc, 32);
    const double cc = finish_score(PCV_METRIC_COSINE, acc[0], gld(&a.norm[la]), gld(&a.norm[lb]));
    if (!(cc >= a.threshold)) return;
    (void)g_atomic_add(&a.degree[la], 1u);
    (void)g_atomic_add(&a.degree[lb], 1u);
    gst(&a.conf[g_atomic_add64(&a.counters[kDensityConfirmed], 1ull)], cd);  // (at most n_cand of them)
}

__global__ __launch_bounds__(256) void density_core_kernel(const DensityArgs a, uint32_t launch_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= launch_rows) return;
    const bool part = gld(&a.rinv[i]) != 0.0f;
    const bool core = part && (unsigned long long)gld(&a.degree[i]) + 1ull >= (unsigned long long)a.min_items;
    gst(&a.core[i], (uint8_t)(core ? 1 : 0));
    gst(&a.parent[i], (uint32_t)i);
    gst(&a.attach[i], kNoRow);
}

// one thread per entry of the confirmed list (as many as the rescore step counted)
__global__ __launch_bounds__(256) void density_link_list_kernel(const DensityArgs a) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= gld(&a.counters[kDensityConfirmed])) return;
    const uint64_t cd = gld(&a.conf[i]);
    const uint32_t la = (uint32_t)(cd >> 32), lb = (uint32_t)cd;
    density_link_pair(a, la, lb, gld(&a.core[la]) != 0, gld(&a.core[lb]) != 0);
}

// root[r]: a core row's root; a border row's: the root of the core row it attaches to; kNoRow otherwise.  rank[r] = 1 for a root
// (the scan that follows turns it into the number of roots before r).  `parent` is final here: plain loads.
__global__ __launch_bounds__(256) void density_flatten_kernel(const DensityArgs a, uint32_t launch_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= launch_rows) return;
    uint32_t x = kNoRow;
    if (gld(&a.core[i]))
        x = (uint32_t)i;
    else if (gld(&a.rinv[i]) != 0.0f)
        x = gld(&a.attach[i]);
    if (x != kNoRow)
        for (uint32_t q = gld(&a.parent[x]); q != x; q = gld(&a.parent[x])) x = q;
    gst(&a.root[i], x);
    gst(&a.rank[i], x == (uint32_t)i ? 1u : 0u);
}

// one workgroup: rank = its exclusive scan, 1024 rows a step (neighbors_offsets_kernel); the total is the number of clusters
__global__ __launch_bounds__(1024) void density_rank_kernel(const DensityArgs a, uint32_t launch_rows) {
    __shared__ uint32_t wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < launch_rows; base += 1024) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t x = i < launch_rows ? gld(&a.rank[i]) : 0u;
        uint32_t inc = x;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(inc, off);
            if (lane >= off) inc += y;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            before += w < wave ? wsum[w] : 0u;
            total += wsum[w];
        }
        if (i < launch_rows) gst(&a.rank[i], carry + before + inc - x);
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) gst(&a.counters[kDensityClusters], (unsigned long long)carry);
}

__global__ __launch_bounds__(256) void density_output_kernel(const ScanParams* __restrict__ pp, const DensityArgs a) {
    const ScanParams& p = *pp;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    int kind = -2;  // a launch row behind its segment's last row
    if (i < (uint64_t)p.total_blocks * 32) {
        const RowRef r = row_ref(p, (uint32_t)i);
        if (r.row < gld(&r.sg->nrows)) {
            const int64_t o = gld(&a.seg_out0[r.sg - p.seg]) + (int64_t)r.row;
            const bool part = gld(&a.rinv[i]) != 0.0f;
            const uint32_t root = gld(&a.root[i]);
            kind = !part ? PCV_DENSITY_NONE : gld(&a.core[i]) ? PCV_DENSITY_CORE : root != kNoRow ? PCV_DENSITY_BORDER : PCV_DENSITY_NOISE;
            gst(&a.out_label[o], root != kNoRow ? (int32_t)gld(&a.rank[root]) : (int32_t)-1);
            gst(&a.out_kind[o], (int8_t)kind);
            gst(&a.out_degree[o], part ? (int32_t)gld(&a.degree[i]) : (int32_t)0);
            gst(&a.out_ids[o], row_id(r));
        }
    }
    // (no early return above: the whole wave votes)
    const unsigned long long n_core = __builtin_popcountll(__ballot(kind == PCV_DENSITY_CORE));
    const unsigned long long n_border = __builtin_popcountll(__ballot(kind == PCV_DENSITY_BORDER));
    const unsigned long long n_noise = __builtin_popcountll(__ballot(kind == PCV_DENSITY_NOISE));
    if ((threadIdx.x & 63) == 0) {
        if (n_core) (void)g_atomic_add64(&a.counters[kDensityCore], n_core);
        if (n_border) (void)g_atomic_add64(&a.counters[kDensityBorder], n_border);
        if (n_noise) (void)g_atomic_add64(&a.counters[kDensityNoise], n_noise);
        if (n_core + n_border + n_noise) (void)g_atomic_add64(&a.counters[kDensityParticipating], n_core + n_border + n_noise);
    }
}

template <bool LINK>
void launch_screen(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t NT = a.tile_blocks;
    PCV_REQUIRE((NT == 1 || NT == 2 || NT == 4) && a.span_blocks >= NT && a.span_blocks < (1u << 15), "density screen: bad tile (%u blocks, spans of %u)", NT,
                a.span_blocks);
    const size_t lds = (size_t)NT * 32 * p.D4 * 4 * sizeof(uint16_t);
    const unsigned tiles = (p.total_blocks + NT - 1) / NT;
    const unsigned spans = (p.total_blocks + a.span_blocks - 1) / a.span_blocks;
    PCV_REQUIRE(spans <= 65535u, "density screen: %u spans", spans);
    const dim3 grid(tiles, spans);
#define PCV_DENSITY(N)                                                          \
    allow_dynamic_lds((const void*)density_screen_kernel<N, LINK>, lds);        \
    density_screen_kernel<N, LINK><<<grid, kScreenWaves * 64, lds, st>>>(dp, a);
    if (NT == 4) {
        PCV_DENSITY(4)
    } else if (NT == 2) {
        PCV_DENSITY(2)
    } else {
        PCV_DENSITY(1)
    }
#undef PCV_DENSITY
    PCV_LAUNCHED();
}

}  // namespace

void launch_density_degree(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a) { launch_screen<false>(st, p, dp, a); }

void launch_density_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a) {
    if (a.n_cand == 0) return;
    density_rescore_kernel<<<cdiv64((int64_t)a.n_cand, 256), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

void launch_density_core(hipStream_t st, const ScanParams& p, const DensityArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t launch_rows = p.total_blocks * 32;
    density_core_kernel<<<cdiv64((int64_t)launch_rows, 256), 256, 0, st>>>(a, launch_rows);
    PCV_LAUNCHED();
}

void launch_density_link(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a) {
    launch_screen<true>(st, p, dp, a);
    if (a.n_cand == 0) return;
    density_link_list_kernel<<<cdiv64((int64_t)a.n_cand, 256), 256, 0, st>>>(a);
    PCV_LAUNCHED();
}

void launch_density_labels(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t launch_rows = p.total_blocks * 32;
    density_flatten_kernel<<<cdiv64((int64_t)launch_rows, 256), 256, 0, st>>>(a, launch_rows);
    density_rank_kernel<<<1, 1024, 0, st>>>(a, launch_rows);
    density_output_kernel<<<cdiv64((int64_t)launch_rows, 256), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

}  // namespace pcv
