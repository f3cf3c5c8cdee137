// linkage_kernels.hip — the device steps of pcv_searcher_linkage_tree (DESIGN.md §4 "Linkage tree"): the single-linkage hierarchy of
// the participating rows, i.e. their maximum spanning tree under the canonical f64 cosine with a strict total order of the edges,
// exact, computed where the rows live, in Borůvka rounds.  The norms come from selfjoin_prep_kernel (launch_selfjoin_prep); a round is
//
//   1. linkage_screen_kernel<NT, false>   the bound pass: the tile-in-LDS, stream-the-blocks screen of neighbors_screen_kernel (a
//                                         further copy of its staging and MFMA loop: that kernel's code object must not move) over
//                                         every stride-th partner block.  Per tile row it keeps the largest certified screening score
//                                         s = acc * rinv_a * rinv_b with a certified partner of ANOTHER component and publishes it
//                                         with an atomic max into comp_max[comp of the row] when the wave's stream ends.
//      linkage_threshold_kernel           thr[root] = comp_max - 2 margin, rounded down (-inf: no bound).
//   2. linkage_screen_kernel<NT, true>    the list pass: the full square.  (owner a, partner b) is a candidate iff both take part,
//                                         s >= thr[comp[a]] (or a row is wild) and comp[a] != comp[b].  The owner's threshold is
//                                         gathered when the tile is staged and lives where the neighbours' per-row one does; the
//                                         components are looked at only for the accumulators that passed the score test, loaded on
//                                         demand inside that rare branch, so the streaming loop holds no register for them.
//   3. linkage_rescore_kernel             one thread per candidate: the canonical f64 cosine (pair_sums and finish_score: the
//                                         arithmetic of selfjoin_rescore_kernel), a 64-bit atomic max of its image into best_key of
//                                         the owner's component.
//      linkage_choose_kernel              candidates that reach their component's best: a 64-bit atomic min of (lower row, higher
//                                         row) into best_pair.  Max and min commute: nothing depends on the order of arrival.
//   4. linkage_merge_kernel               one thread per component with a choice: the edge is emitted unless the component at its
//                                         other end chose the same pair and has the lower root; then the lock-free union of
//                                         density_kernels.hip.
//      linkage_flatten_kernel, _settle    comp = find(row), the count of the components, parent = comp.
// and linkage_rows_kernel / linkage_edges_kernel write the outputs by position when one component is left.
#include "device_access.h"
#include "launch_rows.h"
#include "row_jobs.h"

namespace pcv {
namespace {

constexpr int kLinkWaves = 8;  // waves of a screen workgroup: one tile in LDS per CU, two waves per SIMD
constexpr unsigned long long kNoPair = ~0ull;

__device__ __forceinline__ void g_atomic_max64(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_max((PCV_GLOBAL unsigned long long*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void g_atomic_min64(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_min((PCV_GLOBAL unsigned long long*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// density_find / density_union (density_kernels.hip), word for word: parent[r] <= r at every time, a root is hooked under a lower
// root by a compare-and-swap that expects it to still be a root, nobody waits for anybody, no plain store while the kernel runs.
__device__ __forceinline__ uint32_t linkage_find(const uint32_t* parent, uint32_t x) {
    while (true) {
        const uint32_t q = ld_relaxed(&parent[x]);
        if (q == x) return x;
        x = q;
    }
}
__device__ __forceinline__ void linkage_union(uint32_t* parent, uint32_t a, uint32_t b) {
    while (true) {
        a = linkage_find(parent, a);
        b = linkage_find(parent, b);
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

// grid, tile, stream and accumulator layout: neighbors_screen_kernel.  x = tile (NT consecutive blocks: the owners), y = walk: the
// sampled blocks [y * walk_len, + walk_len) of the launch, cut at its end; sampled block j is launch block j * stride.  Wave w takes
// the sampled blocks first + w, first + w + kLinkWaves, ...  D[row of the streamed block][row of the tile]: lane (c = lane & 31,
// h = lane >> 5) holds tile rows 32 t + c and, in accumulator i, block row (i & 3) + 8 (i >> 2) + 4 h.
template <int NT, bool LIST>
__global__ __launch_bounds__(kLinkWaves * 64) void linkage_screen_kernel(const ScanParams* __restrict__ pp, const LinkageArgs a) {
    const ScanParams& p = *pp;
    extern __shared__ uint4 lq[];  // [NT*32][Dp/8] 16-byte pieces of 8 bf16, swizzled
    __shared__ const float4* tbase[NT];
    const int D4 = p.D4, P8 = D4 >> 1, NCH = D4 >> 4;
    const uint32_t TB = p.total_blocks;
    const uint32_t tb0 = blockIdx.x * NT;
    const uint32_t step = kLinkWaves * a.stride;  // launch blocks between two blocks of a wave
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
    for (int i = threadIdx.x; i < NT * 32 * P8; i += kLinkWaves * 64) {
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
    // ra: rinv of the lane's tile rows (zero behind the launch's last block);  bd: the list pass's threshold of each — that of its
    // component, gathered here — and the bound pass's running maximum of each over the wave's whole stream;  ca: the bound pass's
    // component of each (comp is zero behind the launch's last block, where ra is zero too)
    float ra[NT], bd[NT];
    uint32_t ca[LIST ? 1 : NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const size_t row = (size_t)(tb0 + t) * 32 + c;
        ra[t] = gld(&a.rinv[row]);
        const uint32_t cr = gld(&a.comp[row]);
        bd[t] = LIST ? gld(&a.thr[cr]) : -__builtin_inff();
        if (!LIST) ca[t] = cr;
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
    auto rb_prefetch = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            rb[j] = *(const PCV_GLOBAL f32x4*)(a.rinv + (size_t)cons.gb * 32 + 8 * j + 4 * h);
            if (!LIST) cb[j] = *(const PCV_GLOBAL u32x4*)(a.comp + (size_t)cons.gb * 32 + 8 * j + 4 * h);
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

    auto epilogue = [&]() {
        if (NCH < 2) rb_prefetch();
        if (LIST) {
            uint32_t n = 0;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) n += passes(t, i) ? 1u : 0u;
            if (n) {
                // rare: only here are the components looked at, loaded on demand; the pairs are judged again instead of kept as
                // masks (neighbors_screen_kernel).  A row is of its own component: no pair (a, a) is listed.
                uint32_t nf = 0;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const uint32_t co = gld(&a.comp[owner_row(t)]);
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        if (passes(t, i)) nf += gld(&a.comp[partner_row(i)]) != co ? 1u : 0u;
                }
                if (nf) {
                    unsigned long long at = g_atomic_add64(&a.counters[kLinkListed], nf);
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const uint32_t co = gld(&a.comp[owner_row(t)]);
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            if (passes(t, i) && gld(&a.comp[partner_row(i)]) != co) {
                                if (at < a.cand_cap) gst(&a.cand[at], ((uint64_t)owner_row(t) << 32) | partner_row(i));
                                ++at;
                            }
                        }
                    }
                }
            }
        } else {
            // the running maximum of the certified scores with rows of other components (a wild partner adds nothing)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float m = bd[t];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float rbi = rb[i >> 2][i & 3];
                    const float s = acc[t][i] * ra[t] * rbi;
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

    // one chunk of loads in flight while one feeds the matrix cores (every buf[] index a literal, or the array moves to scratch);
    // the block's rinv values are requested one chunk ahead of the epilogue and before that step's row loads
#define PCV_LINK_STEP(REFILL, CONS)                      \
    if (NCH >= 2 && cons.ch == NCH - 2) rb_prefetch();   \
    produce(buf[REFILL]);                                \
    consume(buf[CONS]);                                  \
    if (cons.gb >= b1) break;
    produce(buf[0]);
    while (true) {
        PCV_LINK_STEP(1, 0)
        PCV_LINK_STEP(0, 1)
    }
#undef PCV_LINK_STEP
    if (!LIST) {
        // the wave's stream has ended: publish.  Max commutes, so comp_max does not depend on which wave lands first.  In the late
        // rounds a few components hold every row and every lane of every wave publishes to the same few words: a lane whose
        // maximum the word already holds (comp_max only rises) leaves the atomic out
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

// comp = parent = the row itself; the participating rows are counted
__global__ __launch_bounds__(256) void linkage_begin_kernel(const LinkageArgs a, uint32_t launch_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool part = false;
    if (i < launch_rows) {
        gst(&a.comp[i], (uint32_t)i);
        gst(&a.parent[i], (uint32_t)i);
        part = gld(&a.rinv[i]) != 0.0f;
    }
    const unsigned long long n = __builtin_popcountll(__ballot(part));  // (no early return above: the whole wave votes)
    if ((threadIdx.x & 63) == 0 && n) (void)g_atomic_add64(&a.counters[kLinkParticipating], n);
}

// cert[root] = 1 where the component has a certified row
__global__ __launch_bounds__(256) void linkage_cert_kernel(const LinkageArgs a, uint32_t launch_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= launch_rows) return;
    if (gld(&a.rinv[i]) > 0.0f) (void)g_atomic_max(&a.cert[gld(&a.comp[i])], 1u);
}

// thr of every root (of every launch row: the entries of the others are never read), and the counts the host's decision to repeat
// a sampled bound pass rests on
__global__ __launch_bounds__(256) void linkage_threshold_kernel(const LinkageArgs a, uint32_t launch_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool certified = false, unbounded = false;
    if (i < launch_rows) {
        float thr = -__builtin_inff();
        if (gld(&a.comp[i]) == (uint32_t)i && gld(&a.rinv[i]) != 0.0f) {
            const uint32_t key = gld(&a.comp_max[i]);
            certified = gld(&a.cert[i]) != 0;
            if (key != 0)
                thr = __double2float_rd((double)key_f32(key) - 2.0 * (double)a.margin);
            else
                unbounded = certified;
        }
        gst(&a.thr[i], thr);
    }
    const unsigned long long nc = __builtin_popcountll(__ballot(certified)), nu = __builtin_popcountll(__ballot(unbounded));
    if ((threadIdx.x & 63) == 0) {
        if (nc) (void)g_atomic_add64(&a.counters[kLinkCertRoots], nc);
        if (nu) (void)g_atomic_add64(&a.counters[kLinkUnbounded], nu);
    }
}

// one thread per candidate: the canonical cosine, its image kept for the choose step and raised into the owner's component
__global__ __launch_bounds__(256) void linkage_rescore_kernel(const ScanParams* __restrict__ pp, const LinkageArgs a) {
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
    const unsigned long long key = cc == cc ? f64_key(cc) : 0ull;  // (both rows have a cosine: c is a number)
    gst(&a.cand_key[i], key);
    if (key) g_atomic_max64(&a.best_key[gld(&a.comp[la])], key);
}

// one thread per candidate: among those that reach their component's best c, the lowest (lower row, higher row)
__global__ __launch_bounds__(256) void linkage_choose_kernel(const LinkageArgs a) {
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

// one thread per launch row; the roots with a choice work.  comp is the round's; only parent changes here.
__global__ __launch_bounds__(256) void linkage_merge_kernel(const LinkageArgs a, uint32_t launch_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= launch_rows) return;
    if (gld(&a.comp[i]) != (uint32_t)i) return;
    const unsigned long long pair = gld(&a.best_pair[i]);
    if (pair == kNoPair) return;
    const uint32_t lo = (uint32_t)(pair >> 32), hi = (uint32_t)pair;
    const uint32_t clo = gld(&a.comp[lo]), chi = gld(&a.comp[hi]);
    const uint32_t other = clo == (uint32_t)i ? chi : clo;
    // a mutual choice is one edge: the component with the lower root emits it
    if (!(gld(&a.best_pair[other]) == pair && other < (uint32_t)i)) {
        const unsigned long long at = g_atomic_add64(&a.counters[kLinkEmitted], 1ull);
        if (at < a.edge_cap) {
            gst(&a.edge_pair[at], pair);
            gst(&a.edge_key[at], gld(&a.best_key[i]));
        }
    }
    linkage_union(a.parent, lo, hi);
}

// `parent` is final here: plain loads.  comp = the root; the roots of participating rows are counted
__global__ __launch_bounds__(256) void linkage_flatten_kernel(const LinkageArgs a, uint32_t launch_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool root = false;
    if (i < launch_rows) {
        uint32_t x = (uint32_t)i;
        for (uint32_t q = gld(&a.parent[x]); q != x; q = gld(&a.parent[x])) x = q;
        gst(&a.comp[i], x);
        root = x == (uint32_t)i && gld(&a.rinv[i]) != 0.0f;
    }
    const unsigned long long n = __builtin_popcountll(__ballot(root));
    if ((threadIdx.x & 63) == 0 && n) (void)g_atomic_add64(&a.counters[kLinkRoots], n);
}

// (a launch of its own: the flatten step still walks the paths this one cuts short)
__global__ __launch_bounds__(256) void linkage_settle_kernel(const LinkageArgs a, uint32_t launch_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= launch_rows) return;
    gst(&a.parent[i], gld(&a.comp[i]));
}

__device__ __forceinline__ int64_t linkage_id(const RowRef& q) {
    const int64_t* ids = gld(&q.sg->ids);
    return ids ? gld(&ids[q.row]) : gld(&q.sg->id0) + (int64_t)q.row;
}

__global__ __launch_bounds__(256) void linkage_rows_kernel(const ScanParams* __restrict__ pp, const LinkageArgs a) {
    const ScanParams& p = *pp;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)p.total_blocks * 32) return;
    const RowRef r = row_ref(p, (uint32_t)i);
    if (r.row >= gld(&r.sg->nrows)) return;
    const int64_t o = gld(&a.seg_out0[r.sg - p.seg]) + (int64_t)r.row;
    gst(&a.out_ids[o], linkage_id(r));
    gst(&a.out_part[o], (int8_t)(gld(&a.rinv[i]) != 0.0f ? 1 : 0));
}

__global__ __launch_bounds__(256) void linkage_edges_kernel(const ScanParams* __restrict__ pp, const LinkageArgs a) {
    const ScanParams& p = *pp;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_edges) return;
    const unsigned long long pair = gld(&a.edge_pair[i]);
    const RowRef ra = row_ref(p, (uint32_t)(pair >> 32)), rb = row_ref(p, (uint32_t)pair);
    LinkEdge e;
    e.c = key_f64(gld(&a.edge_key[i]));
    e.pos_a = gld(&a.seg_out0[ra.sg - p.seg]) + (int64_t)ra.row;
    e.pos_b = gld(&a.seg_out0[rb.sg - p.seg]) + (int64_t)rb.row;
    e.id_a = linkage_id(ra);
    e.id_b = linkage_id(rb);
    PCV_GLOBAL LinkEdge* out = (PCV_GLOBAL LinkEdge*)&a.out_edges[i];
    out->c = e.c;
    out->pos_a = e.pos_a;
    out->pos_b = e.pos_b;
    out->id_a = e.id_a;
    out->id_b = e.id_b;
}

template <bool LIST>
void launch_screen(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t NT = a.tile_blocks;
    PCV_REQUIRE((NT == 1 || NT == 2 || NT == 4) && a.stride >= 1 && a.walk_len >= 1 && (!LIST || a.stride == 1),
                "linkage screen: bad shape (tile of %u blocks, stride %u, walks of %u)", NT, a.stride, a.walk_len);
    const size_t lds = (size_t)NT * 32 * p.D4 * 4 * sizeof(uint16_t);
    const unsigned tiles = (p.total_blocks + NT - 1) / NT;
    const unsigned sampled = (p.total_blocks + a.stride - 1) / a.stride;
    const unsigned walks = (sampled + a.walk_len - 1) / a.walk_len;
    PCV_REQUIRE(walks <= 65535u, "linkage screen: %u walks", walks);
    const dim3 grid(tiles, walks);
#define PCV_LINK(N)                                                             \
    allow_dynamic_lds((const void*)linkage_screen_kernel<N, LIST>, lds);        \
    linkage_screen_kernel<N, LIST><<<grid, kLinkWaves * 64, lds, st>>>(dp, a);
    if (NT == 4) {
        PCV_LINK(4)
    } else if (NT == 2) {
        PCV_LINK(2)
    } else {
        PCV_LINK(1)
    }
#undef PCV_LINK
    PCV_LAUNCHED();
}

}  // namespace

void launch_linkage_begin(hipStream_t st, const ScanParams& p, const LinkageArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t launch_rows = p.total_blocks * 32;
    linkage_begin_kernel<<<cdiv64((int64_t)launch_rows, 256), 256, 0, st>>>(a, launch_rows);
    PCV_LAUNCHED();
}

void launch_linkage_bound(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t launch_rows = p.total_blocks * 32;
    linkage_cert_kernel<<<cdiv64((int64_t)launch_rows, 256), 256, 0, st>>>(a, launch_rows);
    launch_screen<false>(st, p, dp, a);
}

void launch_linkage_threshold(hipStream_t st, const ScanParams& p, const LinkageArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t launch_rows = p.total_blocks * 32;
    linkage_threshold_kernel<<<cdiv64((int64_t)launch_rows, 256), 256, 0, st>>>(a, launch_rows);
    PCV_LAUNCHED();
}

void launch_linkage_list(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a) { launch_screen<true>(st, p, dp, a); }

void launch_linkage_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a) {
    if (a.n_cand == 0) return;
    linkage_rescore_kernel<<<cdiv64((int64_t)a.n_cand, 256), 256, 0, st>>>(dp, a);
    linkage_choose_kernel<<<cdiv64((int64_t)a.n_cand, 256), 256, 0, st>>>(a);
    PCV_LAUNCHED();
}

void launch_linkage_merge(hipStream_t st, const ScanParams& p, const LinkageArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t launch_rows = p.total_blocks * 32;
    const unsigned grid = cdiv64((int64_t)launch_rows, 256);
    linkage_merge_kernel<<<grid, 256, 0, st>>>(a, launch_rows);
    linkage_flatten_kernel<<<grid, 256, 0, st>>>(a, launch_rows);
    linkage_settle_kernel<<<grid, 256, 0, st>>>(a, launch_rows);
    PCV_LAUNCHED();
}

void launch_linkage_output(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a) {
    if (p.total_blocks == 0) return;
    linkage_rows_kernel<<<cdiv64((int64_t)p.total_blocks * 32, 256), 256, 0, st>>>(dp, a);
    if (a.n_edges) linkage_edges_kernel<<<cdiv64((int64_t)a.n_edges, 256), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

}  // namespace pcv
