// grouped_kernels.hip — the id-keyed tables of a searcher (groups, values) and the select step of pcv_searcher_search_grouped
// (DESIGN.md §4 "Grouped results").
//
// A table maps item id -> int64 (a group key, a value): open addressing, capacity a power of two, linear probing from id_hash, kIdEmpty in free
// slots (corpus.h: the definitions the batch tables of hide / update / views use).  The id kIdEmpty itself has no slot: its value
// lives in GroupHead::side_val.  One value of the table, `none`, means "the id has an entry and nothing else": a slot that was never
// stored to reads `none` as well, and the counter of ids follows the transitions none <-> anything else.  The table is instantiated
// twice (corpus.h): the group table with none = kNoGroup (-1; the host admits no other negative group) and the value table of
// DESIGN.md §4 "Item values and filtered search" with none = kNoValue (INT64_MIN).  There are no tombstones: an entry, once made,
// stays until the table is cleared.
//
// Nothing here depends on the order in which an atomic lands:
//   * an upsert is two launches.  group_claim_kernel: every element of the batch finds or claims the slot of its id (64-bit
//     compare-and-swap on the key; whoever loses a race for a free slot sees the winner's key and either has found its own id or
//     probes on) and raises the slot's word of `claim` to its batch index + 1 (atomic max).  group_store_kernel: the one element
//     whose index IS that maximum — the last occurrence of the id in the batch — reads the old value, stores the new one and
//     counts none -> set / set -> none.  Which slot an id lands in may differ from run to run (two ids racing for one free
//     slot), what the table maps it to does not: a probe walks the whole chain up to the first free slot;
//   * group_rehash_kernel moves distinct keys: the same argument, without values in dispute;
//   * grouped_select_kernel only reads the table; its own counters are integer adds in LDS, which commute.
#include "corpus.h"
#include "device_access.h"
#include "group_table.h"
#include "launch_rows.h"
#include "scan.h"

namespace pcv {
namespace {

typedef unsigned long long u64;

__device__ __forceinline__ int64_t key_load(const int64_t* p) {
    return (int64_t)__hip_atomic_load((const PCV_GLOBAL u64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// returns the key found in the slot (== kIdEmpty: the slot is this id's now)
__device__ __forceinline__ int64_t key_claim(int64_t* p, int64_t id) {
    u64 expected = (u64)kIdEmpty;
    __hip_atomic_compare_exchange_strong((PCV_GLOBAL u64*)p, &expected, (u64)id, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (int64_t)expected;
}
__device__ __forceinline__ void count_add(int64_t* p, int64_t v) {
    __hip_atomic_fetch_add((PCV_GLOBAL u64*)p, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void group_fill_kernel(int64_t* __restrict__ keys, int64_t* __restrict__ vals, uint64_t slots, int64_t none) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < slots) {
        gst(&keys[i], kIdEmpty);
        gst(&vals[i], none);
    }
}

// Element i of the batch finds or makes the slot of ids[i] -> slot_of[i] (kGroupSideSlot: the id is kIdEmpty) and bids for it.
__global__ __launch_bounds__(256) void group_claim_kernel(int64_t* __restrict__ keys, uint32_t mask, uint32_t* __restrict__ claim,
                                                          GroupHead* __restrict__ head, const int64_t* __restrict__ ids, uint32_t n,
                                                          uint32_t* __restrict__ slot_of) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = gld(&ids[i]);
    if (id == kIdEmpty) {
        g_atomic_max(&head->side_claim, i + 1);
        gst(&slot_of[i], kGroupSideSlot);
        return;
    }
    uint32_t h = id_hash(id, mask);
    for (;; h = (h + 1) & mask) {
        int64_t k = key_load(&keys[h]);
        if (k == kIdEmpty) {
            k = key_claim(&keys[h], id);
            if (k == kIdEmpty) {
                count_add(&head->entries, 1);
                break;
            }
        }
        if (k == id) break;
    }
    g_atomic_max(&claim[h], i + 1);
    gst(&slot_of[i], h);
}

// The highest bidder of each slot stores its value.
__global__ __launch_bounds__(256) void group_store_kernel(int64_t* __restrict__ vals, uint32_t* __restrict__ claim,
                                                          GroupHead* __restrict__ head, const int64_t* __restrict__ groups, uint32_t n,
                                                          const uint32_t* __restrict__ slot_of, int64_t none) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = gld(&slot_of[i]);
    const int64_t g = gld(&groups[i]);
    int64_t old;
    if (h == kGroupSideSlot) {
        if (gld(&head->side_claim) != i + 1) return;
        old = gld(&head->side_val);
        gst(&head->side_val, g);
        gst(&head->side_claim, 0u);
        if (gld(&head->side_present) == 0) {
            gst(&head->side_present, 1u);
            count_add(&head->entries, 1);
        }
    } else {
        if (gld(&claim[h]) != i + 1) return;
        old = gld(&vals[h]);
        gst(&vals[h], g);
        gst(&claim[h], 0u);  // (the words are all 0 again when the launch is through: the next batch starts from that)
    }
    if (old == none && g != none) count_add(&head->ids, 1);
    if (old != none && g == none) count_add(&head->ids, -1);
}

// Every entry of the old table into the new one (filled with free slots, at least as large).
__global__ __launch_bounds__(256) void group_rehash_kernel(const int64_t* __restrict__ old_keys, const int64_t* __restrict__ old_vals,
                                                           uint64_t old_slots, int64_t* __restrict__ keys, int64_t* __restrict__ vals,
                                                           uint32_t mask) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= old_slots) return;
    const int64_t id = gld(&old_keys[i]);
    if (id == kIdEmpty) return;
    uint32_t h = id_hash(id, mask);
    for (;; h = (h + 1) & mask) {  // (the keys of a table are distinct: a slot taken is another id's)
        if (key_load(&keys[h]) != kIdEmpty) continue;
        if (key_claim(&keys[h], id) == kIdEmpty) break;
    }
    gst(&vals[h], gld(&old_vals[i]));
}

__global__ __launch_bounds__(256) void group_lookup_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ vals, uint32_t mask,
                                                           const GroupHead* __restrict__ head, const int64_t* __restrict__ ids, uint32_t n,
                                                           int64_t* __restrict__ out, int64_t none) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    gst(&out[i], group_of(keys, vals, mask, gld(&head->side_val), gld(&ids[i]), none));
}

// The groups of a row job's launch rows (row_jobs.h, PairGroups), behind its prep step: one thread per launch row.  A row that takes
// no part (rinv == 0) has no group here; the others get what the table holds for their id.  Plain vector stores to grp / tag, one
// integer add per wave to the counter, nothing to the table.
__global__ __launch_bounds__(256) void row_groups_kernel(const ScanParams* __restrict__ pp, const PairGroups a) {
    const ScanParams& p = *pp;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t g = -1;
    const bool in = i < (uint64_t)p.total_blocks * 32;
    if (in && gld(&a.rinv[i]) != 0.0f) g = group_of(a.keys, a.vals, a.mask, a.side_val, row_id(row_ref(p, (uint32_t)i)), kNoGroup);
    if (in) {
        gst(&a.grp[i], g);
        gst(&a.tag[i], group_tag(g));
    }
    const u64 grouped = __ballot(g >= 0);
    if ((threadIdx.x & 63) == 0 && grouped != 0) g_atomic_add64(&a.counters[kPairGroupRows], (unsigned long long)__popcll(grouped));
}

// The select step: one workgroup of kMaxK threads per query, thread t for hit t of the pass's list (p.out, best first; the hits
// of a short list come first).  Hit t is NEW iff it has no group, or its group is neither one of the kept rows of earlier
// passes nor that of a hit before it in this list.  The new hits, in list order, are the kept rows of this pass: a prefix count
// gives each its output slot, and the one that fills slot num_results - 1 is the cut — the walk ends with it, and the hits behind
// it are not examined.  Every examined hit that is not new adds one to the counter of the kept row of its group, which is either
// an older one or a new hit before it (and so before the cut).
__global__ __launch_bounds__(kMaxK) void grouped_select_kernel(const ScanParams* __restrict__ pp, const GroupedArgs a) {
    const ScanParams& p = *pp;
    __shared__ int64_t s_group[kMaxK];      // group of hit t (-1: none)
    __shared__ int64_t s_kept_group[kMaxK]; // groups of the kept rows of earlier passes (-1: none)
    __shared__ int32_t s_count[kMaxK];      // collapsed rows of every kept row, old and new
    __shared__ int32_t s_slot[kMaxK];       // output slot of a new hit
    __shared__ u64 s_new[kMaxK / 64];       // the waves' masks of new hits
    __shared__ uint32_t s_n_new;
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
    if (t == 0) {
        s_n_new = 0;
        s_cut = -1;
    }
    s_kept_group[t] = t < nk0 ? gld(&a.kept_group[o + t]) : (int64_t)-1;
    s_count[t] = t < nk0 ? gld(&a.collapsed[o + t]) : 0;
    const int64_t g = live ? group_of(a.keys, a.vals, a.mask, a.side_val, h.id, kNoGroup) : (int64_t)-1;
    s_group[t] = g;
    __syncthreads();
    if (live) atomicAdd(&s_n_new, 1u);
    int owner_old = -1, owner_hit = -1;  // the kept row of the hit's group: an older one / a hit before it (the first of them)
    if (live && g >= 0) {
        for (int j = 0; j < nk0; ++j)
            if (s_kept_group[j] == g) owner_old = j;  // (at most one: kept groups are distinct)
        if (owner_old < 0)
            for (int u = t - 1; u >= 0; --u)
                if (s_group[u] == g) owner_hit = u;
    }
    const bool is_new = live && owner_old < 0 && owner_hit < 0;
    const u64 mask = __ballot(is_new);
    const int lane = t & 63, wave = t >> 6;
    if (lane == 0) s_new[wave] = mask;
    __syncthreads();
    int slot = nk0 + __popcll(mask & (((u64)1 << lane) - 1));
    for (int w = 0; w < wave; ++w) slot += __popcll(s_new[w]);
    if (is_new) {
        s_slot[t] = slot;
        if (slot == a.num_results - 1) s_cut = t;  // (one hit has that slot, or none)
    }
    __syncthreads();
    const int n_live = (int)s_n_new;
    const int cut = s_cut;                            // -1: the list ends before the num_results-th kept row
    const int last = cut >= 0 ? cut : n_live - 1;     // the last hit examined (-1: the list was empty)
    if (live && t <= last) {
        if (is_new) {
            a.kept[o + slot] = h;
            gst(&a.kept_group[o + slot], g);
        } else {
            atomicAdd(&s_count[owner_old >= 0 ? owner_old : s_slot[owner_hit]], 1);
        }
    }
    __syncthreads();
    int total_new = 0;
    for (int w = 0; w < kMaxK / 64; ++w) total_new += __popcll(s_new[w]);
    const int nk = cut >= 0 ? a.num_results : nk0 + total_new;
    if (t < nk) gst(&a.collapsed[o + t], s_count[t]);
    if (t == max(last, 0)) {
        DistinctRec out;
        out.kept = (uint32_t)nk;
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

void launch_group_fill(hipStream_t st, int64_t* keys, int64_t* vals, uint64_t slots, int64_t none) {
    if (slots == 0) return;
    group_fill_kernel<<<cdiv64((int64_t)slots, 256), 256, 0, st>>>(keys, vals, slots, none);
    PCV_LAUNCHED();
}

void launch_group_upsert(hipStream_t st, int64_t* keys, int64_t* vals, uint32_t mask, uint32_t* claim, GroupHead* head, const int64_t* ids,
                         const int64_t* groups, uint32_t n, uint32_t* slot_of, int64_t none) {
    if (n == 0) return;
    PCV_REQUIRE(keys != nullptr && vals != nullptr && claim != nullptr && (mask & (mask + 1)) == 0 && n <= kGroupBatch,
                "group upsert: bad shape (%u ids, mask %#x)", n, mask);
    const unsigned grid = cdiv64(n, 256);
    group_claim_kernel<<<grid, 256, 0, st>>>(keys, mask, claim, head, ids, n, slot_of);
    PCV_LAUNCHED();
    group_store_kernel<<<grid, 256, 0, st>>>(vals, claim, head, groups, n, slot_of, none);
    PCV_LAUNCHED();
}

void launch_group_rehash(hipStream_t st, const int64_t* old_keys, const int64_t* old_vals, uint64_t old_slots, int64_t* keys, int64_t* vals,
                         uint32_t mask) {
    if (old_slots == 0) return;
    PCV_REQUIRE((mask & (mask + 1)) == 0 && (uint64_t)mask + 1 >= old_slots, "group rehash: %llu slots into %llu",
                (unsigned long long)old_slots, (unsigned long long)mask + 1);
    group_rehash_kernel<<<cdiv64((int64_t)old_slots, 256), 256, 0, st>>>(old_keys, old_vals, old_slots, keys, vals, mask);
    PCV_LAUNCHED();
}

void launch_group_lookup(hipStream_t st, const int64_t* keys, const int64_t* vals, uint32_t mask, const GroupHead* head, const int64_t* ids,
                         uint32_t n, int64_t* out, int64_t none) {
    if (n == 0) return;
    group_lookup_kernel<<<cdiv64(n, 256), 256, 0, st>>>(keys, vals, mask, head, ids, n, out, none);
    PCV_LAUNCHED();
}

void launch_row_groups(hipStream_t st, const ScanParams& p, const ScanParams* dp, const PairGroups& a) {
    if (p.total_blocks == 0) return;
    PCV_REQUIRE(a.keys == nullptr || (a.mask & (a.mask + 1)) == 0, "row groups: mask %#x", a.mask);
    row_groups_kernel<<<cdiv64((int64_t)p.total_blocks * 32, 256), 256, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

void launch_grouped_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const GroupedArgs& a) {
    PCV_REQUIRE(p.B > 0 && p.k >= 1 && p.k <= kMaxK && a.num_results >= 1 && a.num_results <= kMaxK,
                "grouped select: bad shape (%d queries, lists of %d, %d results)", p.B, p.k, a.num_results);
    grouped_select_kernel<<<p.B, kMaxK, 0, st>>>(dp, a);
    PCV_LAUNCHED();
}

}  // namespace pcv
