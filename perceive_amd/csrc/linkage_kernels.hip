// linkage_kernels.hip — the device steps of pcv_searcher_linkage_tree (DESIGN.md §4 "Linkage tree"): the single-linkage hierarchy of
// the participating rows, i.e. their maximum spanning tree under the canonical f64 cosine with a strict total order of the edges,
// exact, computed where the rows live, in Borůvka rounds.  The norms come from selfjoin_prep_kernel (launch_selfjoin_prep); a round is
//
//   1. linkage_screen_kernel<NT, false>   the bound pass: the tile-in-LDS, stream-the-blocks screen of pair_screen.h (DESIGN.md §4
//                                         "The row-pair screen") on the grid of neighbors_screen_kernel, over
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
//                                         launch_rows.h.
//      linkage_flatten_kernel, _settle    comp = find(row), the count of the components, parent = comp.
// and linkage_rows_kernel / linkage_edges_kernel write the outputs by position when one component is left.
// The reach tree (reach_kernels.hip) runs the same rounds with the cap applied: the screen's third template flag, and the cert and
// choose steps as they are.
#include "device_access.h"
#include "launch_rows.h"
#include "pair_screen.h"
#include "row_jobs.h"

namespace pcv {
namespace {

constexpr unsigned long long kNoPair = ~0ull;

// The epilogues of the linkage screen and, CAP, of the reach screen (the mutual-reachability weight min(s, core of the owner, core of
// the partner): klo / khi are each launch row's core rounded down / up to f32, reach_kernels.hip).
//   bd: the list pass's threshold of each of the lane's tile rows — that of its component, gathered when the stream begins; CAP: +inf
//       where the owner's khi is below it (no edge of the owner can be the component's best) — and the bound pass's running maximum
//       of each over the wave's whole stream
//   ca, ka: the bound pass's component and klo of each tile row (comp is zero behind the launch's last block, where ra is zero too)
//   cb, kb: the bound pass's components and klo of the streamed block's rows, beside rb
template <int NT, bool LIST, bool CAP>
struct LinkPolicy {
    const LinkageArgs& a;
    const float* cap;  // CAP: klo of every launch row (the bound pass), khi (the list pass)
    float bd[NT];
    uint32_t ca[LIST ? 1 : NT];
    float ka[!LIST && CAP ? NT : 1];
    u32x4 cb[LIST ? 1 : 4];
    f32x4 kb[!LIST && CAP ? 4 : 1];
    __device__ __forceinline__ void begin(uint32_t tb0, int c) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const size_t row = (size_t)(tb0 + t) * 32 + c;
            const uint32_t cr = gld(&a.comp[row]);
            if (LIST) {
                const float th = gld(&a.thr[cr]);
                bd[t] = !CAP || gld(&cap[row]) >= th ? th : __builtin_inff();
            } else {
                bd[t] = -__builtin_inff();
                ca[t] = cr;
                if (CAP) ka[t] = gld(&cap[row]);
            }
        }
    }
    __device__ __forceinline__ void prefetch(uint32_t gb, int h, int j) {
        if (LIST) return;
        cb[j] = *(const PCV_GLOBAL u32x4*)(a.comp + (size_t)gb * 32 + 8 * j + 4 * h);
        if (CAP) kb[j] = *(const PCV_GLOBAL f32x4*)(cap + (size_t)gb * 32 + 8 * j + 4 * h);
    }
    __device__ __forceinline__ void block(const f32x16 (&acc)[NT], const float (&ra)[NT], const f32x4 (&rb)[4], const PairWhere& at) {
        if (LIST) {
            // (owner 32 t + c of the tile, partner i of the block) passes the score test
            auto passes = [&](int t, int i) -> bool {
                const float rbi = rb[i >> 2][i & 3];
                const float s = acc[t][i] * ra[t] * rbi;
                return (ra[t] > 0.0f && rbi > 0.0f) ? s >= bd[t] : (ra[t] != 0.0f && rbi != 0.0f);  // (a wild row: every pair, scan.h)
            };
            // the partner is of another component (a row is of its own: no pair (a, a) is listed) and, CAP, its khi reaches the owner's
            // threshold (bd is +inf for an owner that failed its own test: no finite khi reaches that)
            auto foreign = [&](int t, int i, uint32_t co) -> bool {
                const uint32_t pr = at.partner_row(i);
                return gld(&a.comp[pr]) != co && (!CAP || gld(&cap[pr]) >= bd[t]);
            };
            uint32_t n = 0;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) n += passes(t, i) ? 1u : 0u;
            if (n == 0) return;
            // rare: only here are the components looked at, loaded on demand, so the streaming loop holds no register for them; the
            // pairs are judged again instead of kept as masks (neighbors_screen_kernel)
            uint32_t nf = 0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const uint32_t co = gld(&a.comp[at.owner_row(t)]);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (passes(t, i)) nf += foreign(t, i, co) ? 1u : 0u;
            }
            if (nf == 0) return;
            unsigned long long k = g_atomic_add64(&a.counters[kLinkListed], nf);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const uint32_t co = gld(&a.comp[at.owner_row(t)]);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (passes(t, i) && foreign(t, i, co)) {
                        if (k < a.cand_cap) gst(&a.cand[k], ((uint64_t)at.owner_row(t) << 32) | at.partner_row(i));
                        ++k;
                    }
                }
            }
        } else {
            // the running maximum of the certified scores — CAP: of min(s, klo of the owner, klo of the partner) — with rows of other
            // components (a wild partner adds nothing)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float m = bd[t];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float rbi = rb[i >> 2][i & 3];
                    if (rbi > 0.0f) {  // a certified partner
                        // (the empty statement keeps this a branch, as in the capped form, where the compiler leaves one by itself:
                        // folded into selects, the uncapped pass waits for every load in flight before its first compare and
                        // measured 3 to 5 % slower — DESIGN.md §4 "The row-pair screen")
                        if (!CAP) asm volatile("");
                        float s = acc[t][i] * ra[t] * rbi;
                        if (CAP) s = fminf(s, fminf(ka[t], kb[i >> 2][i & 3]));
                        m = cb[i >> 2][i & 3] != ca[t] ? fmaxf(m, s) : m;
                    }
                }
                bd[t] = m;
            }
        }
    }
    // The wave's stream has ended: the bound pass publishes.  Max commutes, so comp_max does not depend on which wave lands first.  In
    // the late rounds a few components hold every row and every lane of every wave publishes to the same few words: a lane whose
    // maximum the word already holds (comp_max only rises) leaves the atomic out
    __device__ __forceinline__ void end(const float (&ra)[NT], int, int h) {
        if (LIST) return;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float m = fmaxf(bd[t], __shfl_xor(bd[t], 32));
            if (h == 0 && ra[t] > 0.0f && m > -__builtin_inff()) {
                const uint32_t key = f32_key(m);
                if (ld_relaxed(&a.comp_max[ca[t]]) < key) (void)g_atomic_max(&a.comp_max[ca[t]], key);
            }
        }
    }
};

// grid: neighbors_screen_kernel's.  x = tile (NT consecutive blocks: the owners), y = walk: the sampled blocks [y * walk_len,
// + walk_len) of the launch, cut at its end; sampled block j is launch block j * stride.  Wave w takes the sampled blocks first + w,
// first + w + kScreenWaves, ...  Staging, stream and accumulator layout: pair_screen.h.
template <int NT, bool LIST, bool CAP>
__device__ __forceinline__ void link_screen(const ScanParams& p, const LinkageArgs& a, const float* cap) {
    extern __shared__ uint4 lq[];
    __shared__ const float4* tbase[NT];
    const uint32_t TB = p.total_blocks;
    const uint32_t tb0 = blockIdx.x * NT;
    const uint32_t step = kScreenWaves * a.stride;  // launch blocks between two blocks of a wave
    const uint32_t SB = (TB + a.stride - 1) / a.stride;
    const uint64_t first = (uint64_t)blockIdx.y * a.walk_len;
    if (first >= SB) return;  // (the whole workgroup)
    const uint32_t b0 = (uint32_t)first * a.stride;
    const uint32_t b1 = (uint32_t)min((uint64_t)SB, first + a.walk_len) * a.stride;  // every sampled block below it is below TB
    pair_stage_tile<NT>(p, lq, tbase, tb0);
    const uint32_t wave = uniform(threadIdx.x >> 6);
    if (b0 + wave * a.stride >= b1) return;
    LinkPolicy<NT, LIST, CAP> pol{a, cap};
    pair_stream<NT>(p, lq, a.rinv, tb0, b0 + wave * a.stride, b1, step, pol);
}
// two thin kernels: the uncapped forms keep the linkage tree's kernel arguments
template <int NT, bool LIST>
__global__ __launch_bounds__(kScreenWaves * 64) void linkage_screen_kernel(const ScanParams* __restrict__ pp, const LinkageArgs a) {
    link_screen<NT, LIST, false>(*pp, a, nullptr);
}
template <int NT, bool LIST>
__global__ __launch_bounds__(kScreenWaves * 64) void reach_screen_kernel(const ScanParams* __restrict__ pp, const LinkageArgs a, const float* cap) {
    link_screen<NT, LIST, true>(*pp, a, cap);
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
    row_union(a.parent, lo, hi);
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

__global__ __launch_bounds__(256) void linkage_rows_kernel(const ScanParams* __restrict__ pp, const LinkageArgs a) {
    const ScanParams& p = *pp;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)p.total_blocks * 32) return;
    const RowRef r = row_ref(p, (uint32_t)i);
    if (r.row >= gld(&r.sg->nrows)) return;
    const int64_t o = gld(&a.seg_out0[r.sg - p.seg]) + (int64_t)r.row;
    gst(&a.out_ids[o], row_id(r));
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
    e.id_a = row_id(ra);
    e.id_b = row_id(rb);
    PCV_GLOBAL LinkEdge* out = (PCV_GLOBAL LinkEdge*)&a.out_edges[i];
    out->c = e.c;
    out->pos_a = e.pos_a;
    out->pos_b = e.pos_b;
    out->id_a = e.id_a;
    out->id_b = e.id_b;
}

template <bool LIST, bool CAP>
void launch_screen(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a, const float* cap) {
    if (p.total_blocks == 0) return;
    const char* what = CAP ? "reach" : "linkage";
    const uint32_t NT = a.tile_blocks;
    PCV_REQUIRE((NT == 1 || NT == 2 || NT == 4) && a.stride >= 1 && a.walk_len >= 1 && (!LIST || a.stride == 1),
                "%s screen: bad shape (tile of %u blocks, stride %u, walks of %u)", what, NT, a.stride, a.walk_len);
    const size_t lds = (size_t)NT * 32 * p.D4 * 4 * sizeof(uint16_t);
    const unsigned tiles = (p.total_blocks + NT - 1) / NT;
    const unsigned sampled = (p.total_blocks + a.stride - 1) / a.stride;
    const unsigned walks = (sampled + a.walk_len - 1) / a.walk_len;
    PCV_REQUIRE(walks <= 65535u, "%s screen: %u walks", what, walks);
    const dim3 grid(tiles, walks);
#define PCV_LINK(N)                                                                            \
    if constexpr (CAP) {                                                                       \
        allow_dynamic_lds((const void*)reach_screen_kernel<N, LIST>, lds);                     \
        reach_screen_kernel<N, LIST><<<grid, kScreenWaves * 64, lds, st>>>(dp, a, cap);        \
    } else {                                                                                   \
        allow_dynamic_lds((const void*)linkage_screen_kernel<N, LIST>, lds);                   \
        linkage_screen_kernel<N, LIST><<<grid, kScreenWaves * 64, lds, st>>>(dp, a);           \
    }
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

void launch_linkage_bound(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a, const float* klo) {
    if (p.total_blocks == 0) return;
    const uint32_t launch_rows = p.total_blocks * 32;
    linkage_cert_kernel<<<cdiv64((int64_t)launch_rows, 256), 256, 0, st>>>(a, launch_rows);
    if (klo)
        launch_screen<false, true>(st, p, dp, a, klo);
    else
        launch_screen<false, false>(st, p, dp, a, nullptr);
}

void launch_linkage_threshold(hipStream_t st, const ScanParams& p, const LinkageArgs& a) {
    if (p.total_blocks == 0) return;
    const uint32_t launch_rows = p.total_blocks * 32;
    linkage_threshold_kernel<<<cdiv64((int64_t)launch_rows, 256), 256, 0, st>>>(a, launch_rows);
    PCV_LAUNCHED();
}

void launch_linkage_list(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a, const float* khi) {
    if (khi)
        launch_screen<true, true>(st, p, dp, a, khi);
    else
        launch_screen<true, false>(st, p, dp, a, nullptr);
}

void launch_linkage_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a) {
    if (a.n_cand == 0) return;
    linkage_rescore_kernel<<<cdiv64((int64_t)a.n_cand, 256), 256, 0, st>>>(dp, a);
    launch_linkage_choose(st, a);
}

void launch_linkage_choose(hipStream_t st, const LinkageArgs& a) {
    if (a.n_cand == 0) return;
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
