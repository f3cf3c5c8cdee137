// neighbors_kernels.hip — the device steps of pcv_searcher_neighbors and pcv_searcher_match (DESIGN.md §4 "Item neighbours", "Item
// matches"): for every participating owner row its k best other participating partner rows by the canonical f64 cosine, exact,
// computed where the rows live.  The owners are the launch blocks [owner_block0, total_blocks), the partners [0, partner_blocks)
// (NeighborArgs): the whole launch twice for the neighbours, the suffix and the prefix of a launch ordered [to only | to and from |
// from only] for the matches.  The norms come from selfjoin_prep_kernel (launch_selfjoin_prep); then
//
//   1. neighbors_screen_kernel<NT, false>   the bound pass: the tile-in-LDS, stream-the-blocks screen of selfjoin_screen_kernel over a
//                                           SAMPLE of the partner blocks (every stride-th), cut into spans.  Per tile row and span it
//                                           leaves the largest certified screening score s = acc * rinv_a * rinv_b (span_max).
//   2. neighbors_threshold_kernel           a wave per owner: thr = (k-th largest span maximum) - 2 margin, and under a score bound at
//                                           least min_score - margin.  The spans are disjoint
//                                           partner sets, so k maxima are k distinct partners with c >= s - margin: the k-th best c
//                                           of the row is >= kth_s - margin, and a member of the true top k has s >= kth_s - 2 margin.
//   3. neighbors_screen_kernel<NT, true>    the list pass: the same stream over ALL partner blocks, the full rectangle.  (owner a, partner b) is
//                                           a candidate iff both take part, a != b and s >= thr[a] — a threshold per tile row, in
//                                           registers beside rinv_a.  Appends past the list's capacity are counted, not stored: the
//                                           host repeats the launch once with the capacity the count asks for.
//   4. count / offsets / rescore            candidates per owner, their exclusive scan, and one thread per candidate: the canonical
//                                           f64 cosine (pair_sums and finish_score: the arithmetic of selfjoin_rescore_kernel), its
//                                           f64_key image (0 below the score bound) and the partner stored in the owner's stretch.
//   5. neighbors_select_kernel              a wave per owner: k rounds, each the best entry (c descending, position ascending) strictly
//                                           behind the one picked before — no entry is changed, so the order the atomics of step 4
//                                           landed in cannot show.  It writes ids, neighbour ids, (float)c and counts.
// The grouped calls (pcv_searcher_neighbors_grouped, _match_grouped; DESIGN.md §4 "Group-aware pairs") run the same steps with the
// rows' groups beside them (row_jobs.h, PairGroups): the GROUPS form of the bound pass leaves the owner's siblings out of the maxima and
// publishes 64-bit images that carry the tag of the arg-max, the grouped threshold kernel takes k maxima of k different groups, the
// list pass is the plain one, and the GROUPS forms of rescore and select decide siblings on the 64-bit keys.
#include <algorithm>

#include "device_access.h"
#include "launch_rows.h"
#include "pair_screen.h"
#include "row_jobs.h"

namespace pcv {
namespace {

__device__ __forceinline__ void g_atomic_max32(uint32_t* p, uint32_t v) {
    (void)__hip_atomic_fetch_max((PCV_GLOBAL uint32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t g_atomic_add32(uint32_t* p, uint32_t v) {
    return __hip_atomic_fetch_add((PCV_GLOBAL uint32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The epilogues of the neighbour screen.  bd: the list pass's threshold of each of the lane's tile rows, the bound pass's running
// maximum of each over the blocks of the span so far.  step and b1 are the stream's: the bound pass publishes when the wave's next
// block lies in another span.
// GROUPS (the bound pass of the grouped calls, DESIGN.md §4 "Group-aware pairs"): what the policy keeps beside bd.  own: the tag of
// each of the lane's tile rows under kGroupsSkipOwn, else 0 — a partner carrying it adds nothing to the maximum;  best: the tag of
// the partner the running maximum came from;  partner: the tags of the block's rows in the layout of rb.
template <int NT, bool GROUPS>
struct NeighborTags {};
template <int NT>
struct NeighborTags<NT, true> {
    uint32_t own[NT], best[NT];
    u32x4 partner[4];
};

template <int NT, bool LIST, bool GROUPS = false>
struct NeighborPolicy {
    static_assert(!(LIST && GROUPS), "the list pass has no grouped form: siblings above thr are listed and the f64 step drops them");
    const NeighborArgs& a;
    uint32_t owner_rows, step, b1;  // owner_rows: the launch's, the stride of span_max
    float bd[NT];
    NeighborTags<NT, GROUPS> g;
    __device__ __forceinline__ void begin(uint32_t tb0, int c) {
#pragma unroll
        for (int t = 0; t < NT; ++t) bd[t] = LIST ? gld(&a.thr[(size_t)(tb0 + t) * 32 + c]) : -__builtin_inff();
        if constexpr (GROUPS) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                g.own[t] = (a.group_flags & kGroupsSkipOwn) ? gld(&a.tag[(size_t)(tb0 + t) * 32 + c]) : 0u;
                g.best[t] = 0u;
            }
        }
    }
    __device__ __forceinline__ void prefetch(uint32_t gb, int h, int j) {
        if constexpr (GROUPS) g.partner[j] = *(const PCV_GLOBAL u32x4*)(a.tag + (size_t)gb * 32 + 8 * j + 4 * h);
    }
    __device__ __forceinline__ void end(const float (&)[NT], int, int) {}
    __device__ __forceinline__ void block(const f32x16 (&acc)[NT], const float (&ra)[NT], const f32x4 (&rb)[4], const PairWhere& at) {
        const bool own = at.gb >= at.tb0 && at.gb < at.tb0 + NT;  // the block is one of the tile's own: a row is no partner of itself
        if (LIST) {
            // (owner 32 t + c of the tile, partner i of the block) is a candidate
            auto passes = [&](int t, int i) -> bool {
                const float rbi = rb[i >> 2][i & 3];
                const float s = acc[t][i] * ra[t] * rbi;
                bool ok = (ra[t] > 0.0f && rbi > 0.0f) ? s >= bd[t] : (ra[t] != 0.0f && rbi != 0.0f);  // (a wild row: every pair, scan.h)
                if (own) ok = ok && at.owner_row(t) != at.partner_row(i);
                return ok;
            };
            uint32_t n = 0;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) n += passes(t, i) ? 1u : 0u;
            if (n) {  // rare; the pairs are judged again instead of kept as masks: four registers the <4> form does not have
                unsigned long long k = g_atomic_add64(&a.counters[0], n);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        if (passes(t, i)) {
                            if (k < a.cand_cap) gst(&a.cand[k], ((uint64_t)at.owner_row(t) << 32) | at.partner_row(i));
                            ++k;
                        }
                    }
                }
            }
        } else if constexpr (GROUPS) {
            // as below, without the owner's siblings, and with the tag of the partner the maximum came from.  A foreign partner whose
            // tag collides with the owner's is left out too: the maximum stays a lower bound
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float m = bd[t];
                uint32_t mt = g.best[t];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float rbi = rb[i >> 2][i & 3];
                    const uint32_t pt = g.partner[i >> 2][i & 3];
                    const float s = acc[t][i] * ra[t] * rbi;
                    bool ok = rbi > 0.0f && !(g.own[t] != 0u && pt == g.own[t]);
                    if (own) ok = ok && at.owner_row(t) != at.partner_row(i);
                    const bool up = ok && s > m;
                    m = up ? s : m;
                    mt = up ? pt : mt;
                }
                bd[t] = m;
                g.best[t] = mt;
            }
            const uint32_t per = a.stride * a.span_len;
            const uint32_t span = at.gb / per, next = at.gb + step;
            if (next >= b1 || next / per != span) {  // publish: max commutes on the 64-bit images too; on equal scores either tag is a witness
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float mo = __shfl_xor(bd[t], 32);
                    const uint32_t to = __shfl_xor(g.best[t], 32);
                    const bool take = mo > bd[t];
                    const float m = take ? mo : bd[t];
                    const uint32_t mt = take ? to : g.best[t];
                    if (at.h == 0 && ra[t] > 0.0f && m > -__builtin_inff())
                        g_atomic_max64(&a.span_max64[(size_t)span * owner_rows + (size_t)(at.tb0 - a.owner_block0 + t) * 32 + at.c],
                                       ((unsigned long long)f32_key(m) << 32) | mt);
                    bd[t] = -__builtin_inff();
                    g.best[t] = 0u;
                }
            }
        } else {
            // the running maximum of the certified scores: partners that take part with a certified s (a wild partner adds nothing)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float m = bd[t];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float rbi = rb[i >> 2][i & 3];
                    const float s = acc[t][i] * ra[t] * rbi;
                    bool ok = rbi > 0.0f;
                    if (own) ok = ok && at.owner_row(t) != at.partner_row(i);
                    m = ok ? fmaxf(m, s) : m;
                }
                bd[t] = m;
            }
            // the wave's next block lies in another span, or there is none: publish.  Max commutes, so span_max does not depend on
            // which wave lands first
            const uint32_t per = a.stride * a.span_len;  // launch blocks a span covers
            const uint32_t span = at.gb / per, next = at.gb + step;
            if (next >= b1 || next / per != span) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float m = fmaxf(bd[t], __shfl_xor(bd[t], 32));
                    if (at.h == 0 && ra[t] > 0.0f && m > -__builtin_inff())
                        g_atomic_max32(&a.span_max[(size_t)span * owner_rows + (size_t)(at.tb0 - a.owner_block0 + t) * 32 + at.c], f32_key(m));
                    bd[t] = -__builtin_inff();
                }
            }
        }
    }
};

// grid: x = tile (NT consecutive blocks from owner_block0 on: the owners), y = walk: the sampled blocks [y * walk_len, + walk_len) of
// the partner blocks, cut at their end; sampled block j is launch block j * stride.  Wave w takes the sampled blocks first + w, first + w + kScreenWaves, ...
// Staging, stream and accumulator layout: pair_screen.h.
template <int NT, bool LIST, bool GROUPS = false>
__global__ __launch_bounds__(kScreenWaves * 64) void neighbors_screen_kernel(const ScanParams* __restrict__ pp, const NeighborArgs a) {
    const ScanParams& p = *pp;
    extern __shared__ uint4 lq[];
    __shared__ const float4* tbase[NT];
    const uint32_t PB = a.partner_blocks;
    const uint32_t tb0 = a.owner_block0 + blockIdx.x * NT;
    const uint32_t step = kScreenWaves * a.stride;  // launch blocks between two blocks of a wave
    const uint32_t SB = (PB + a.stride - 1) / a.stride;
    const uint64_t first = (uint64_t)blockIdx.y * a.walk_len;
    if (first >= SB) return;  // (the whole workgroup)
    const uint32_t b0 = (uint32_t)first * a.stride;
    const uint32_t b1 = (uint32_t)min((uint64_t)SB, first + a.walk_len) * a.stride;  // every sampled block below it is below PB
    pair_stage_tile<NT>(p, lq, tbase, tb0);
    const uint32_t wave = uniform(threadIdx.x >> 6);
    if (b0 + wave * a.stride >= b1) return;
    NeighborPolicy<NT, LIST, GROUPS> pol{a, (p.total_blocks - a.owner_block0) * 32, step, b1};
    pair_stream<NT>(p, lq, a.rinv, tb0, b0 + wave * a.stride, b1, step, pol);
}

// a wave per owner row: the k-th largest of the row's span maxima, found bit by bit from the top on their order-preserving images
// (the largest T with at least k images >= T; 0 when fewer than k are defined), less twice the margin, rounded down.  Under a score
// bound no partner with s < min_score - margin can have c >= min_score: the threshold is at least that, also where T is 0.
__global__ __launch_bounds__(256) void neighbors_threshold_kernel(const NeighborArgs a, uint32_t owner_rows) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= owner_rows) return;  // (the whole wave)
    const int lane = threadIdx.x & 63;
    uint32_t v[kMaxNeighborSpans / 64];
#pragma unroll
    for (int j = 0; j < (int)(kMaxNeighborSpans / 64); ++j) {
        const uint32_t sp = (uint32_t)j * 64 + lane;
        v[j] = sp < a.spans ? gld(&a.span_max[(size_t)sp * owner_rows + row]) : 0u;
    }
    uint32_t T = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = T | (1u << bit);
        int n = 0;
#pragma unroll
        for (int j = 0; j < (int)(kMaxNeighborSpans / 64); ++j) n += __builtin_popcountll(__ballot(v[j] >= cand));
        if (n >= a.k) T = cand;
    }
    if (lane != 0) return;
    const uint32_t lr = a.owner_block0 * 32 + row;
    float thr = -__builtin_inff();
    if (gld(&a.rinv[lr]) > 0.0f) {
        if (T != 0) thr = __double2float_rd((double)key_f32(T) - 2.0 * (double)a.margin);
        if (a.min_score != -1.0f) thr = fmaxf(thr, __double2float_rd((double)a.min_score - (double)a.margin));
    }
    gst(&a.thr[lr], thr);
}

// The grouped form (group_flags != 0; DESIGN.md §4 "Group-aware pairs"): a wave per owner row over the row's 64-bit span images, k
// rounds.  A round takes the largest remaining image — of equal ones the one in the lowest lane, then the lowest register, so that
// exactly one is retired — and, under kGroupsOnePerGroup, retires every remaining image with its non-zero tag as well.  T is the
// score image of the k-th taken (0: fewer): the k taken are partners of k disjoint spans in k different groups (or singletons), none
// a sibling of the owner under kGroupsSkipOwn.  With every tag 0 the k-th taken is the k-th largest: the plain kernel's T.
__global__ __launch_bounds__(256) void neighbors_threshold_grouped_kernel(const NeighborArgs a, uint32_t owner_rows) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= owner_rows) return;  // (the whole wave)
    const int lane = threadIdx.x & 63;
    constexpr int NV = (int)(kMaxNeighborSpans / 64);
    unsigned long long v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const uint32_t sp = (uint32_t)j * 64 + lane;
        v[j] = sp < a.spans ? gld(&a.span_max64[(size_t)sp * owner_rows + row]) : 0ull;
    }
    const bool one_per = (a.group_flags & kGroupsOnePerGroup) != 0;
    uint32_t T = 0;
    for (int n = 0; n < a.k; ++n) {
        unsigned long long mine = 0;
#pragma unroll
        for (int j = 0; j < NV; ++j) mine = v[j] > mine ? v[j] : mine;
        unsigned long long best = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long o = shfl_xor_u64(best, off);
            best = o > best ? o : best;
        }
        if (best == 0) {  // (wave-uniform) fewer than k
            T = 0;
            break;
        }
        T = (uint32_t)(best >> 32);
        const unsigned long long holders = __ballot(mine == best);
        const bool first = lane == __builtin_ctzll(holders);
        const uint32_t tag = (uint32_t)best;
        bool gone = false;  // the lane's first register holding `best` goes; the others stay unless their tag retires them
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const bool hit = first && !gone && v[j] == best;
            gone = gone || hit;
            const bool same_group = one_per && tag != 0u && v[j] != 0 && (uint32_t)v[j] == tag;
            v[j] = (hit || same_group) ? 0ull : v[j];
        }
    }
    if (lane != 0) return;
    const uint32_t lr = a.owner_block0 * 32 + row;
    float thr = -__builtin_inff();
    if (gld(&a.rinv[lr]) > 0.0f) {
        if (T != 0) thr = __double2float_rd((double)key_f32(T) - 2.0 * (double)a.margin);
        if (a.min_score != -1.0f) thr = fmaxf(thr, __double2float_rd((double)a.min_score - (double)a.margin));
    }
    gst(&a.thr[lr], thr);
}

// one thread per candidate: its owner has one more
__global__ __launch_bounds__(256) void neighbors_count_kernel(const NeighborArgs a) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_cand) return;
    (void)g_atomic_add32(&a.row_cnt[(uint32_t)(gld(&a.cand[i]) >> 32)], 1u);
}

// one workgroup: row_off = the exclusive scan of row_cnt, 1024 rows a step; row_off[n] = the total
__global__ __launch_bounds__(1024) void neighbors_offsets_kernel(const NeighborArgs a, uint32_t launch_rows) {
    __shared__ uint32_t wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < launch_rows; base += 1024) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t x = i < launch_rows ? gld(&a.row_cnt[i]) : 0u;
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
        if (i < launch_rows) gst(&a.row_off[i], carry + before + inc - x);
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) gst(&a.row_off[launch_rows], carry);
}

// one thread per candidate: the canonical cosine, stored with the partner's order row in a slot of the owner's stretch (the image 0
// where c is below the call's score bound: the f64 comparison the screen cannot make).  row_cnt counts down: which slot a candidate
// gets depends on the order the atomics land in, what the select step reads from the stretch does not.
// GROUPS (the grouped calls): the partner's group goes beside sorted_row, and under kGroupsSkipOwn a sibling of the owner — decided on
// the 64-bit keys, never on the tags: a collision would drop a true neighbour — gets the image 0 and is counted, a wave's at a time.
template <bool GROUPS>
__global__ __launch_bounds__(256) void neighbors_rescore_kernel(const ScanParams* __restrict__ pp, const NeighborArgs a) {
    const ScanParams& p = *pp;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if constexpr (GROUPS) {
        bool sibling = false;
        if (i < a.n_cand) {
            const uint64_t cd = gld(&a.cand[i]);
            const uint32_t la = (uint32_t)(cd >> 32), lb = (uint32_t)cd;
            const RowRef ra = row_ref(p, la), rb = row_ref(p, lb);
            const float4* y[1] = {rb.x};
            double acc[1];
            pair_sums<1>(ra.x, y, p.D4, acc, 32);
            const double cc = finish_score(PCV_METRIC_COSINE, acc[0], gld(&a.norm[la]), gld(&a.norm[lb]));
            const uint32_t slot = gld(&a.row_off[la]) + g_atomic_add32(&a.row_cnt[la], 0xffffffffu) - 1u;
            const bool in_bound = a.min_score == -1.0f || cc >= (double)a.min_score;
            const int64_t ga = gld(&a.grp[la]), gb = gld(&a.grp[lb]);
            sibling = (a.group_flags & kGroupsSkipOwn) != 0 && ga >= 0 && ga == gb;
            gst(&a.sorted_key[slot], (cc == cc && in_bound && !sibling) ? f64_key(cc) : 0ull);
            gst(&a.sorted_row[slot], gld(&a.seg_ord0[rb.sg - p.seg]) + rb.row);
            gst(&a.sorted_grp[slot], gb);
        }
        const unsigned long long dropped = __ballot(sibling), active = __ballot(true);
        if (dropped != 0 && (int)(threadIdx.x & 63) == __builtin_ctzll(active))
            g_atomic_add64(&a.gcounters[kPairGroupSiblings], (unsigned long long)__builtin_popcountll(dropped));
        return;
    }
    if (i >= a.n_cand) return;
    const uint64_t cd = gld(&a.cand[i]);
    const uint32_t la = (uint32_t)(cd >> 32), lb = (uint32_t)cd;
    const RowRef ra = row_ref(p, la), rb = row_ref(p, lb);
    const float4* y[1] = {rb.x};
    double acc[1];
    pair_sums<1>(ra.x, y, p.D4, acc, 32);
    const double cc = finish_score(PCV_METRIC_COSINE, acc[0], gld(&a.norm[la]), gld(&a.norm[lb]));
    const uint32_t slot = gld(&a.row_off[la]) + g_atomic_add32(&a.row_cnt[la], 0xffffffffu) - 1u;
    const bool in_bound = a.min_score == -1.0f || cc >= (double)a.min_score;
    gst(&a.sorted_key[slot], (cc == cc && in_bound) ? f64_key(cc) : 0ull);  // (both rows have a cosine: c is a number)
    gst(&a.sorted_row[slot], gld(&a.seg_ord0[rb.sg - p.seg]) + rb.row);
}

// The row behind an order row (row_jobs.h): the last segment in position order whose first order row is not above it.
__device__ __forceinline__ RowRef ord_ref(const ScanParams& p, const NeighborArgs& a, uint32_t orow) {
    int lo = 0, hi = p.nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (gld(&a.seg_ord0[gld(&a.ord_seg[mid])]) <= orow)
            lo = mid;
        else
            hi = mid - 1;
    }
    const uint32_t si = gld(&a.ord_seg[lo]);
    const SegDesc* sg = &p.seg[si];
    const uint32_t row = orow - gld(&a.seg_ord0[si]);
    return {sg, row, gld(&sg->blk) + (size_t)(row >> 5) * p.D4 * 32 + (row & 31)};
}

// (key descending, partner ascending by order row, which is by global position): x comes before y
__device__ __forceinline__ bool nbr_before(unsigned long long kx, uint32_t rx, unsigned long long ky, uint32_t ry) {
    return kx > ky || (kx == ky && rx < ry);
}

// a wave per owner row.  An owner's entries are distinct (a partner is listed once per owner), so "the best entry strictly behind
// the last pick" walks them in order without marking any.
// GROUPS (the grouped calls): the picks' groups are written too, and under kGroupsOnePerGroup the walk passes over every entry whose
// group >= 0 is that of a pick: the round behind a pick marks the entries of its group (kRetired in sorted_grp, in the wave's own
// stretch; each lane re-reads only what it wrote itself) — they all lie behind that pick, which was the best of its group.  The marked
// entries in front of the last pick are the ones the walk passed over: `collapsed`.
constexpr int64_t kRetired = -2;
template <bool GROUPS>
__global__ __launch_bounds__(256) void neighbors_select_kernel(const ScanParams* __restrict__ pp, const NeighborArgs a) {
    const ScanParams& p = *pp;
    const uint32_t lr = a.owner_block0 * 32 + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (lr >= p.total_blocks * 32) return;  // (the whole wave)
    const int lane = threadIdx.x & 63;
    const RowRef r = row_ref(p, lr);
    if (r.row >= gld(&r.sg->nrows)) return;
    const int64_t o = gld(&a.seg_out0[r.sg - p.seg]) + (int64_t)r.row;
    const uint32_t e0 = gld(&a.row_off[lr]), e1 = gld(&a.row_off[lr + 1]);
    unsigned long long last_key = ~0ull;  // (no image is all ones: that would be a NaN)
    uint32_t last_row = 0;
    int64_t last_grp = -1;  // GROUPS under kGroupsOnePerGroup: the group of the last pick
    const bool one_per = GROUPS && (a.group_flags & kGroupsOnePerGroup) != 0;
    int n = 0;
    for (; n < a.k; ++n) {
        unsigned long long bk = 0;
        uint32_t br = 0xffffffffu;
        int64_t bg = -1;
        for (uint32_t e = e0 + lane; e < e1; e += 64) {
            const unsigned long long key = gld(&a.sorted_key[e]);
            const uint32_t row = gld(&a.sorted_row[e]);
            if (key != 0 && nbr_before(last_key, last_row, key, row)) {
                int64_t ge = -1;
                if constexpr (GROUPS) {
                    ge = gld(&a.sorted_grp[e]);
                    if (ge == kRetired) continue;
                    if (one_per && ge >= 0 && ge == last_grp) {
                        gst(&a.sorted_grp[e], kRetired);
                        continue;
                    }
                }
                if (nbr_before(key, row, bk, br)) {
                    bk = key;
                    br = row;
                    bg = ge;
                }
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long ok = __shfl_xor(bk, off);
            const uint32_t orow = __shfl_xor(br, off);
            int64_t og = -1;
            if constexpr (GROUPS) og = (int64_t)shfl_xor_u64((unsigned long long)bg, off);
            if (nbr_before(ok, orow, bk, br)) {
                bk = ok;
                br = orow;
                bg = og;
            }
        }
        if (bk == 0) break;  // (wave-uniform after the exchange)
        last_key = bk;
        last_row = br;
        if (one_per) last_grp = bg;
        if (lane == 0) {
            gst(&a.out_nbr[o * a.k + n], row_id(ord_ref(p, a, br)));
            gst(&a.out_score[o * a.k + n], (float)key_f64(bk));
            if constexpr (GROUPS) gst(&a.out_grp[o * a.k + n], bg);
        }
    }
    for (int j = n + lane; j < a.k; j += 64) {
        gst(&a.out_nbr[o * a.k + j], (int64_t)-1);
        gst(&a.out_score[o * a.k + j], __builtin_nanf(""));
        if constexpr (GROUPS) gst(&a.out_grp[o * a.k + j], (int64_t)-1);
    }
    if (lane == 0) {
        gst(&a.out_ids[o], row_id(r));
        gst(&a.out_count[o], (int32_t)n);
    }
    if constexpr (GROUPS) {
        if (one_per) {  // the entries passed over: marked, and in front of the last pick (a walk that ran out of entries saw them all)
            uint32_t mine = 0;
            for (uint32_t e = e0 + lane; e < e1; e += 64)
                if (gld(&a.sorted_grp[e]) == kRetired && (n < a.k || nbr_before(gld(&a.sorted_key[e]), gld(&a.sorted_row[e]), last_key, last_row))) ++mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) mine += __shfl_xor(mine, off);
            if (lane == 0 && mine != 0) g_atomic_add64(&a.gcounters[kPairGroupCollapsed], (unsigned long long)mine);
        }
    }
}

// GROUPS: the bound pass of a grouped call.  Sixteen partner tags and two tags per tile row beside the <4> form's 248 registers do
// not fit: its tile is two blocks at most (thresholds do not depend on the tile; DESIGN.md §4 "Group-aware pairs").
template <bool LIST, bool GROUPS = false>
void launch_screen(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a) {
    if (a.owner_block0 >= p.total_blocks || a.partner_blocks == 0) return;
    const uint32_t NT = GROUPS ? std::min<uint32_t>(a.tile_blocks, 2u) : a.tile_blocks;
    PCV_REQUIRE(!GROUPS || (a.tag != nullptr && a.span_max64 != nullptr && a.group_flags != 0), "neighbors screen: the grouped bound pass without tags");
    PCV_REQUIRE(a.partner_blocks <= p.total_blocks, "neighbors screen: %u partner blocks of %u", a.partner_blocks, p.total_blocks);
    PCV_REQUIRE((NT == 1 || NT == 2 || NT == 4) && a.stride >= 1 && a.span_len >= 1 && a.walk_len >= 1 && (LIST ? a.stride == 1 : a.spans <= kMaxNeighborSpans),
                "neighbors screen: bad shape (tile of %u blocks, stride %u, spans of %u, walks of %u)", NT, a.stride, a.span_len, a.walk_len);
    const size_t lds = (size_t)NT * 32 * p.D4 * 4 * sizeof(uint16_t);
    const unsigned tiles = (p.total_blocks - a.owner_block0 + NT - 1) / NT;
    const unsigned sampled = (a.partner_blocks + a.stride - 1) / a.stride;
    const unsigned walks = (sampled + a.walk_len - 1) / a.walk_len;
    PCV_REQUIRE(walks <= 65535u, "neighbors screen: %u walks", walks);
    PCV_REQUIRE(LIST || (sampled + a.span_len - 1) / a.span_len == a.spans, "neighbors screen: %u spans of %u for %u sampled blocks", a.spans, a.span_len, sampled);
    const dim3 grid(tiles, walks);
#define PCV_NBR(N)                                                                        \
    allow_dynamic_lds((const void*)neighbors_screen_kernel<N, LIST, GROUPS>, lds);        \
    neighbors_screen_kernel<N, LIST, GROUPS><<<grid, kScreenWaves * 64, lds, st>>>(dp, a);
    if (NT == 4) {
        if constexpr (!GROUPS) {
            PCV_NBR(4)
        }
    } else if (NT == 2) {
        PCV_NBR(2)
    } else {
        PCV_NBR(1)
    }
#undef PCV_NBR
    PCV_LAUNCHED();
}

}  // namespace

void launch_neighbors_bound(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a) {
    if (a.group_flags != 0)
        launch_screen<false, true>(st, p, dp, a);
    else
        launch_screen<false>(st, p, dp, a);
}

void launch_neighbors_list(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a) { launch_screen<true>(st, p, dp, a); }

void launch_neighbors_threshold(hipStream_t st, const ScanParams& p, const NeighborArgs& a) {
    if (a.owner_block0 >= p.total_blocks) return;
    PCV_REQUIRE(a.spans >= 1 && a.spans <= kMaxNeighborSpans && a.k >= 1, "neighbors threshold: %u spans, k = %d", a.spans, a.k);
    const uint32_t owner_rows = (p.total_blocks - a.owner_block0) * 32;
    if (a.group_flags != 0)
        neighbors_threshold_grouped_kernel<<<cdiv64((int64_t)owner_rows, 4), 256, 0, st>>>(a, owner_rows);
    else
        neighbors_threshold_kernel<<<cdiv64((int64_t)owner_rows, 4), 256, 0, st>>>(a, owner_rows);
    PCV_LAUNCHED();
}

void launch_neighbors_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a) {
    if (p.total_blocks == 0) return;
    if (a.n_cand) neighbors_count_kernel<<<cdiv64((int64_t)a.n_cand, 256), 256, 0, st>>>(a);
    neighbors_offsets_kernel<<<1, 1024, 0, st>>>(a, p.total_blocks * 32);
    if (a.n_cand && a.grp != nullptr)
        neighbors_rescore_kernel<true><<<cdiv64((int64_t)a.n_cand, 256), 256, 0, st>>>(dp, a);
    else if (a.n_cand)
        neighbors_rescore_kernel<false><<<cdiv64((int64_t)a.n_cand, 256), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

void launch_owner_offsets(hipStream_t st, const uint64_t* cand, unsigned long long n_cand, uint32_t* row_cnt, uint32_t* row_off, uint32_t launch_rows) {
    NeighborArgs a{};
    a.cand = const_cast<uint64_t*>(cand);  // (read only)
    a.n_cand = n_cand;
    a.row_cnt = row_cnt;
    a.row_off = row_off;
    if (n_cand) neighbors_count_kernel<<<cdiv64((int64_t)n_cand, 256), 256, 0, st>>>(a);
    neighbors_offsets_kernel<<<1, 1024, 0, st>>>(a, launch_rows);
    PCV_LAUNCHED();
}

void launch_neighbors_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a) {
    if (a.owner_block0 >= p.total_blocks) return;
    const unsigned grid = cdiv64((int64_t)(p.total_blocks - a.owner_block0) * 32, 4);
    if (a.grp != nullptr)
        neighbors_select_kernel<true><<<grid, 256, 0, st>>>(dp, a);
    else
        neighbors_select_kernel<false><<<grid, 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

}  // namespace pcv
