// Drives neighbors_grouped, match_grouped, find_duplicates_grouped and last_pair_group_stats of the C++ host mirror
// (include/perceive.hpp) on the GPU: 200 items of 64 features in four planted clusters (cluster = i % 4), the group of item i being
// i % 8 — every cluster holds two groups.  With SKIP_OWN no neighbour is of the owner's group; with ONE_PER_GROUP the seven neighbours
// are one of every other group, the other group of the owner's cluster first; flags 0 is the plain table; without a table the grouped
// calls are the plain ones; sibling pairs leave the duplicate join and are counted.
#include <cmath>
#include <cstdio>
#include <random>
#include <set>

#include "perceive.hpp"

using namespace perceive;

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static bool same_table(const NeighborTable& a, const NeighborTable& b) {
    if (!(a.ids == b.ids && a.neighbor_ids == b.neighbor_ids && a.counts == b.counts && a.scores.size() == b.scores.size())) return false;
    for (size_t i = 0; i < a.scores.size(); ++i)
        if (!(a.scores[i] == b.scores[i] || (std::isnan(a.scores[i]) && std::isnan(b.scores[i])))) return false;
    return true;
}

int main() {
    Context ctx(0);
    const int D = 64, N = 200;
    std::mt19937 rng(77);
    std::normal_distribution<float> nd;
    std::vector<float> centres((size_t)4 * D);
    for (auto& v : centres) v = nd(rng);
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> ids, groups, some;
    for (int i = 0; i < N; ++i) {
        std::vector<float> e(D);
        for (int f = 0; f < D; ++f) e[f] = centres[(size_t)(i % 4) * D + f] + 0.2f * nd(rng);
        rows.push_back({9000 + i, 1 + i % 2, serialize_embedding(e)});
        ids.push_back(9000 + i);
        groups.push_back(i % 8);
        if (i < 120) some.push_back(9000 + i);
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Cosine);
    const NeighborTable plain = s->neighbors({1, 2}, 7);
    // no table: every flag gives the plain table, every partner is a singleton
    for (uint32_t flags = 0; flags < 4; ++flags) {
        const GroupedNeighborTable g = s->neighbors_grouped({1, 2}, 7, flags);
        EXPECT(same_table(g.table, plain));
        for (int64_t x : g.groups) EXPECT(x == PCV_NO_GROUP);
        EXPECT(s->last_pair_group_stats().flags == flags && s->last_pair_group_stats().grouped_rows == 0);
    }
    s->set_groups(ids, groups);
    const GroupedNeighborTable zero = s->neighbors_grouped({1, 2}, 7, 0);
    EXPECT(same_table(zero.table, plain));
    for (size_t i = 0; i < zero.groups.size(); ++i) EXPECT(zero.groups[i] == (zero.table.neighbor_ids[i] - 9000) % 8);
    // SKIP_OWN: seven neighbours of the owner's cluster, none of its group
    const GroupedNeighborTable skip = s->neighbors_grouped({1, 2}, 7);
    EXPECT(skip.table.ids.size() == (size_t)N && skip.groups.size() == (size_t)N * 7);
    for (size_t r = 0; r < skip.table.ids.size(); ++r) {
        const int64_t own = (skip.table.ids[r] - 9000) % 8;
        EXPECT(skip.table.counts[r] == 7);
        for (size_t j = 0; j < 7; ++j) {
            const int64_t m = skip.table.neighbor_ids[r * 7 + j];
            EXPECT(skip.groups[r * 7 + j] == (m - 9000) % 8 && skip.groups[r * 7 + j] != own && (m - 9000) % 4 == own % 4);
        }
    }
    pcv_pair_group_stats st = s->last_pair_group_stats();
    EXPECT(st.flags == PCV_GROUPS_SKIP_OWN && st.grouped_rows == N && st.sibling_candidates > 0 && st.collapsed == 0 && st.bound_tile_rows == 64);
    EXPECT(s->last_neighbor_stats().rows == N && s->last_neighbor_stats().k == 7);
    // both flags: one neighbour of each of the seven other groups, the other group of the owner's cluster first
    const GroupedNeighborTable one = s->neighbors_grouped({1, 2}, 7, PCV_GROUPS_SKIP_OWN | PCV_GROUPS_ONE_PER_GROUP);
    for (size_t r = 0; r < one.table.ids.size(); ++r) {
        const int64_t own = (one.table.ids[r] - 9000) % 8;
        std::set<int64_t> seen(one.groups.begin() + (std::ptrdiff_t)(r * 7), one.groups.begin() + (std::ptrdiff_t)(r * 7 + 7));
        EXPECT(one.table.counts[r] == 7 && seen.size() == 7 && seen.count(own) == 0 && one.groups[r * 7] == (own + 4) % 8);
        EXPECT(one.table.neighbor_ids[r * 7] == skip.table.neighbor_ids[r * 7]);
    }
    EXPECT(s->last_pair_group_stats().collapsed > 0);
    // the matches: the square is the neighbours' table; a rectangle keeps the flags
    const GroupedNeighborTable sq = s->match_grouped({1, 2}, {1, 2}, 7);
    EXPECT(same_table(sq.table, skip.table) && sq.groups == skip.groups);
    const GroupedNeighborTable rect = s->match_grouped({1}, {2}, 3, -1.0f, PCV_GROUPS_ONE_PER_GROUP);
    EXPECT(rect.table.ids.size() == (size_t)N / 2 && s->last_match_stats().rows == N / 2);
    for (size_t r = 0; r < rect.table.ids.size(); ++r) {
        std::set<int64_t> seen(rect.groups.begin() + (std::ptrdiff_t)(r * 3), rect.groups.begin() + (std::ptrdiff_t)(r * 3 + 3));
        EXPECT(rect.table.counts[r] == 3 && seen.size() == 3);
        for (int64_t gk : seen) EXPECT(gk % 2 == 1);  // (source 2 holds the odd items: the odd groups)
    }
    EXPECT(s->match_grouped({}, {1}, 3).table.ids.empty());
    // duplicate pairs: total + skipped is the plain total, no sibling pair is left
    int64_t total = 0, gtotal = 0, skipped = 0;
    s->find_duplicates({1, 2}, 0.8f, 1 << 20, &total);
    const std::vector<DuplicatePair> pairs = s->find_duplicates_grouped({1, 2}, 0.8f, 1 << 20, &gtotal, &skipped);
    EXPECT(total > 0 && skipped > 0 && gtotal + skipped == total && (int64_t)pairs.size() == gtotal);
    for (const DuplicatePair& p : pairs) EXPECT((p.id_a - 9000) % 8 != (p.id_b - 9000) % 8);
    EXPECT(s->last_pair_group_stats().sibling_candidates == skipped && s->last_pair_group_stats().flags == PCV_GROUPS_SKIP_OWN);
    // a view reads its parent's table
    SearcherView v = s->view(some);
    const GroupedNeighborTable vg = v.neighbors_grouped({1, 2}, 5);
    EXPECT(vg.table.ids.size() == 120);
    for (size_t r = 0; r < vg.table.ids.size(); ++r)
        for (size_t j = 0; j < 5; ++j) EXPECT(vg.groups[r * 5 + j] != (vg.table.ids[r] - 9000) % 8 && vg.table.neighbor_ids[r * 5 + j] < 9120);
    EXPECT(v.last_pair_group_stats().grouped_rows == 120);
    if (failures == 0) std::printf("pair_groups_mirror_test: ok\n");
    return failures == 0 ? 0 : 1;
}
