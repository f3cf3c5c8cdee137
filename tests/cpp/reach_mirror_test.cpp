// Drives Searcher::reach_tree, SearcherView::reach_tree and linkage_select of the C++ host mirror (include/perceive.hpp) on the GPU
// with one case the Python test computed with its reference:
//     reach_mirror_test <rows.f32> <n> <dim> <min_items> <edges> <min_cluster_size> <clusters>
//                       then per row: <part> <bits of core, hex> <label of the selection>,
//                       then per edge: <pos_a> <pos_b> <bits of w, hex> <bits of c, hex>, then per cluster: <bits of S, hex> <size>
// The rows come from the raw little-endian f32 file, the ids are 5000 + 3 * position, everything in source 1.  Ids, part, the bits of
// the cores, the edges and the bits of their w and c, the labels, the stabilities and the sizes must be equal; then min_items = 1
// against Searcher::linkage_tree, an empty filter, a source without rows, and a view of the even positions.
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

static uint64_t bits_of(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

int main(int argc, char** argv) {
    if (argc < 8) return 2;
    const int n = std::atoi(argv[2]), dim = std::atoi(argv[3]), min_items = std::atoi(argv[4]), edges = std::atoi(argv[5]);
    const int min_cluster_size = std::atoi(argv[6]), clusters = std::atoi(argv[7]);
    if (argc != 8 + 3 * n + 4 * edges + 2 * clusters) return 2;
    std::vector<float> all((size_t)n * dim);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(all.data(), sizeof(float), all.size(), f) != all.size()) return 2;
    std::fclose(f);

    Context ctx(0);
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> even;
    for (int i = 0; i < n; ++i) {
        rows.push_back({5000 + 3 * i, 1, serialize_embedding(std::vector<float>(all.begin() + (size_t)i * dim, all.begin() + (size_t)(i + 1) * dim))});
        if (i % 2 == 0) even.push_back(5000 + 3 * i);
    }
    auto s = Searcher::build(ctx, rows, dim, Metric::Cosine);
    const ReachTree got = s->reach_tree({1}, min_items);
    EXPECT((int)got.ids.size() == n && got.part.size() == got.ids.size() && got.core.size() == got.ids.size());
    EXPECT((int)got.w.size() == edges && got.c.size() == got.w.size() && got.pos_a.size() == got.w.size() && got.pos_b.size() == got.w.size() &&
           got.id_a.size() == got.w.size() && got.id_b.size() == got.w.size());
    const LinkageSelection sel = linkage_select(got, min_cluster_size);
    EXPECT((int)sel.stability.size() == clusters && (int)sel.size.size() == clusters && sel.labels.size() == got.ids.size());
    int64_t participating = 0;
    for (int i = 0; i < n && i < (int)got.ids.size(); ++i) {
        const char* const* a = argv + 8 + 3 * i;
        EXPECT(got.ids[i] == 5000 + 3 * i);
        EXPECT(got.part[i] == std::atoi(a[0]));
        EXPECT(bits_of(got.core[i]) == std::strtoull(a[1], nullptr, 16) || (got.core[i] != got.core[i] && got.part[i] == 0));
        EXPECT(sel.labels[i] == std::atoi(a[2]));
        participating += got.part[i] != 0;
    }
    for (int i = 0; i < edges && i < (int)got.w.size(); ++i) {
        const char* const* a = argv + 8 + 3 * n + 4 * i;
        EXPECT(got.pos_a[i] == std::atoll(a[0]) && got.pos_b[i] == std::atoll(a[1]));
        EXPECT(bits_of(got.w[i]) == std::strtoull(a[2], nullptr, 16));
        EXPECT(bits_of(got.c[i]) == std::strtoull(a[3], nullptr, 16));
        EXPECT(got.id_a[i] == 5000 + 3 * got.pos_a[i] && got.id_b[i] == 5000 + 3 * got.pos_b[i]);
    }
    for (int k = 0; k < clusters && k < (int)sel.size.size(); ++k) {
        const char* const* a = argv + 8 + 3 * n + 4 * edges + 2 * k;
        EXPECT(bits_of(sel.stability[k]) == std::strtoull(a[0], nullptr, 16));
        EXPECT(sel.size[k] == std::atoll(a[1]));
    }
    const pcv_reach_stats st = s->last_reach_stats();
    EXPECT(st.rows == n && st.participating == participating && st.edges == edges && st.edges == (participating > 0 ? participating - 1 : 0));
    EXPECT(st.rounds >= (participating >= 2 ? 1 : 0) && st.min_items == min_items);
    // min_items = 1 is the linkage tree, and the selection takes either
    const ReachTree one = s->reach_tree({1}, 1);
    const LinkageTree plain = s->linkage_tree({1});
    EXPECT(one.pos_a == plain.pos_a && one.pos_b == plain.pos_b && one.w.size() == plain.c.size());
    for (size_t i = 0; i < one.w.size() && i < plain.c.size(); ++i) EXPECT(bits_of(one.w[i]) == bits_of(plain.c[i]) && bits_of(one.c[i]) == bits_of(plain.c[i]));
    const LinkageSelection a = linkage_select(one, min_cluster_size, true), b = linkage_select(plain, min_cluster_size, true);
    EXPECT(a.labels == b.labels && a.size == b.size && a.stability == b.stability && !a.size.empty());
    EXPECT(s->reach_tree({}, min_items).ids.empty());   // an empty filter selects nothing
    EXPECT(s->reach_tree({2}, min_items).ids.empty());  // ... and so does a source without rows
    SearcherView v = s->view(even);
    const ReachTree vs = v.reach_tree({1}, min_items);
    EXPECT(vs.ids.size() == even.size());
    int64_t vpart = 0;
    for (size_t i = 0; i < vs.ids.size(); ++i) {
        EXPECT(vs.ids[i] == even[i]);  // only the view's items, in the parent's order
        EXPECT(vs.part[i] == got.part[2 * i]);
        if (vs.part[i]) EXPECT(vs.core[i] <= got.core[2 * i]);  // fewer partners: a core can only get worse
        vpart += vs.part[i] != 0;
    }
    EXPECT((int64_t)vs.w.size() == (vpart > 0 ? vpart - 1 : 0));
    EXPECT(v.last_reach_stats().rows == (int64_t)even.size());
    if (failures == 0) std::printf("reach_mirror_test: ok\n");
    return failures == 0 ? 0 : 1;
}
