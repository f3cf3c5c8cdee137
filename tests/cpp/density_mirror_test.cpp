// Drives Searcher::density_clusters and SearcherView::density_clusters of the C++ host mirror (include/perceive.hpp) on the GPU with
// one case the Python test computed with its reference:
//     density_mirror_test <rows.f32> <n> <dim> <threshold bits, hex> <min_items> <clusters> then per row: <label> <kind> <degree>
// The rows come from the raw little-endian f32 file, the ids are 5000 + 3 * position, everything in source 1.  Ids, labels, kinds,
// degrees and the number of clusters must be equal; then an empty filter, a source without rows, and a view of the even positions.
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

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    const int n = std::atoi(argv[2]), dim = std::atoi(argv[3]);
    const uint32_t tbits = (uint32_t)std::strtoul(argv[4], nullptr, 16);
    float threshold;
    std::memcpy(&threshold, &tbits, 4);
    const int min_items = std::atoi(argv[5]), clusters = std::atoi(argv[6]);
    if (argc != 7 + 3 * n) return 2;
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
    const DensityClusters got = s->density_clusters({1}, threshold, min_items);
    EXPECT((int)got.ids.size() == n && got.labels.size() == got.ids.size() && got.kinds.size() == got.ids.size() && got.degrees.size() == got.ids.size());
    EXPECT(got.clusters == clusters);
    int64_t core = 0, border = 0, noise = 0;
    for (int i = 0; i < n && i < (int)got.ids.size(); ++i) {
        const char* const* a = argv + 7 + 3 * i;
        EXPECT(got.ids[i] == 5000 + 3 * i);
        EXPECT(got.labels[i] == std::atoi(a[0]));
        EXPECT(got.kinds[i] == std::atoi(a[1]));
        EXPECT(got.degrees[i] == std::atoi(a[2]));
        core += got.kinds[i] == PCV_DENSITY_CORE;
        border += got.kinds[i] == PCV_DENSITY_BORDER;
        noise += got.kinds[i] == PCV_DENSITY_NOISE;
    }
    const pcv_density_stats st = s->last_density_stats();
    EXPECT(st.rows == n && st.clusters == clusters && st.core == core && st.border == border && st.noise == noise);
    EXPECT(st.participating == core + border + noise);
    EXPECT(s->density_clusters({}, threshold, min_items).ids.empty());   // an empty filter selects nothing
    EXPECT(s->density_clusters({2}, threshold, min_items).ids.empty());  // ... and so does a source without rows
    SearcherView v = s->view(even);
    const DensityClusters vs = v.density_clusters({1}, threshold, min_items);
    EXPECT(vs.ids.size() == even.size());
    for (size_t i = 0; i < vs.ids.size(); ++i) {
        EXPECT(vs.ids[i] == even[i]);                      // only the view's items, in the parent's order
        EXPECT(vs.degrees[i] <= got.degrees[2 * i]);       // fewer partners: the degrees can only drop
    }
    EXPECT(v.last_density_stats().rows == (int64_t)even.size());
    if (failures == 0) std::printf("density_mirror_test: ok\n");
    return failures == 0 ? 0 : 1;
}
