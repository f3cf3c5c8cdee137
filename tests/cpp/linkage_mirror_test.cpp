// Drives Searcher::linkage_tree, SearcherView::linkage_tree and linkage_cut of the C++ host mirror (include/perceive.hpp) on the GPU
// with one case the Python test computed with its reference:
//     linkage_mirror_test <rows.f32> <n> <dim> <edges> <threshold bits of the cut, hex, f64> <clusters of the cut>
//                         then per row: <part> <label of the cut>, then per edge: <pos_a> <pos_b> <bits of c, hex>
// The rows come from the raw little-endian f32 file, the ids are 5000 + 3 * position, everything in source 1.  Ids, part, the edges
// and the bits of their c, the labels and the number of clusters must be equal; then an empty filter, a source without rows, the K
// form of the cut, and a view of the even positions.
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
    if (argc < 7) return 2;
    const int n = std::atoi(argv[2]), dim = std::atoi(argv[3]), edges = std::atoi(argv[4]);
    const uint64_t tbits = std::strtoull(argv[5], nullptr, 16);
    double threshold;
    std::memcpy(&threshold, &tbits, 8);
    const int clusters = std::atoi(argv[6]);
    if (argc != 7 + 2 * n + 3 * edges) return 2;
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
    const LinkageTree got = s->linkage_tree({1});
    EXPECT((int)got.ids.size() == n && got.part.size() == got.ids.size());
    EXPECT((int)got.c.size() == edges && got.pos_a.size() == got.c.size() && got.pos_b.size() == got.c.size() && got.id_a.size() == got.c.size() &&
           got.id_b.size() == got.c.size());
    const LinkageCut cut = linkage_cut(got, threshold);
    EXPECT(cut.clusters == clusters && cut.labels.size() == got.ids.size());
    int64_t participating = 0;
    for (int i = 0; i < n && i < (int)got.ids.size(); ++i) {
        const char* const* a = argv + 7 + 2 * i;
        EXPECT(got.ids[i] == 5000 + 3 * i);
        EXPECT(got.part[i] == std::atoi(a[0]));
        EXPECT(cut.labels[i] == std::atoi(a[1]));
        participating += got.part[i] != 0;
    }
    for (int i = 0; i < edges && i < (int)got.c.size(); ++i) {
        const char* const* a = argv + 7 + 2 * n + 3 * i;
        EXPECT(got.pos_a[i] == std::atoll(a[0]) && got.pos_b[i] == std::atoll(a[1]));
        EXPECT(bits_of(got.c[i]) == std::strtoull(a[2], nullptr, 16));
        EXPECT(got.id_a[i] == 5000 + 3 * got.pos_a[i] && got.id_b[i] == 5000 + 3 * got.pos_b[i]);
    }
    const pcv_linkage_stats st = s->last_linkage_stats();
    EXPECT(st.rows == n && st.participating == participating && st.edges == edges && st.edges == (participating > 0 ? participating - 1 : 0));
    EXPECT(st.rounds >= (participating >= 2 ? 1 : 0));
    for (int64_t K = 1; K <= 3 && K <= participating; ++K) EXPECT(linkage_cut(got, -1.0 / 0.0, K).clusters == K);  // the K form
    EXPECT(s->linkage_tree({}).ids.empty());   // an empty filter selects nothing
    EXPECT(s->linkage_tree({2}).ids.empty());  // ... and so does a source without rows
    SearcherView v = s->view(even);
    const LinkageTree vs = v.linkage_tree({1});
    EXPECT(vs.ids.size() == even.size());
    int64_t vpart = 0;
    for (size_t i = 0; i < vs.ids.size(); ++i) {
        EXPECT(vs.ids[i] == even[i]);            // only the view's items, in the parent's order
        EXPECT(vs.part[i] == got.part[2 * i]);
        vpart += vs.part[i] != 0;
    }
    EXPECT((int64_t)vs.c.size() == (vpart > 0 ? vpart - 1 : 0));
    if (!vs.c.empty() && !got.c.empty()) EXPECT(vs.c[0] <= got.c[0]);  // fewer partners: the best edge can only get worse
    EXPECT(v.last_linkage_stats().rows == (int64_t)even.size());
    if (failures == 0) std::printf("linkage_mirror_test: ok\n");
    return failures == 0 ? 0 : 1;
}
