// Drives Searcher::moments, principal_axes and project (and SearcherView's) of the C++ host mirror (include/perceive.hpp) on the GPU
// with one case the Python test computed with its reference:
//     moments_mirror_test <n> <dim> <participating> <m> <rows.f32> <sums.i64> <cov.f64> <axes.f32> <offsets.f64> <coords.f32>
// The rows come from the raw little-endian files, the ids are 5000 + 3 * position, everything in source 1.  The int64 sums, the f64
// bits of the centred matrix and the f32 bits of the coordinates must be equal; then the eigen-solver, the principal axes, an empty
// filter and a view of the even positions.
#include <cmath>
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

template <class T>
static std::vector<T> read_file(const char* path, size_t count) {
    std::vector<T> v(count);
    FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(T), count, f) != count) {
        std::printf("cannot read %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 11) return 2;
    const size_t n = (size_t)std::atoll(argv[1]), dim = (size_t)std::atoll(argv[2]), m = (size_t)std::atoll(argv[4]);
    const int64_t participating = std::atoll(argv[3]);
    const auto all = read_file<float>(argv[5], n * dim);
    const auto sums = read_file<int64_t>(argv[6], dim);
    const auto cov = read_file<double>(argv[7], dim * dim);
    const auto axes = read_file<float>(argv[8], m * dim);
    const auto offsets = read_file<double>(argv[9], m);
    const auto coords = read_file<float>(argv[10], n * m);

    Context ctx(0);
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> even;
    for (size_t i = 0; i < n; ++i) {
        rows.push_back({5000 + 3 * (int64_t)i, 1, serialize_embedding(std::vector<float>(all.begin() + i * dim, all.begin() + (i + 1) * dim))});
        if (i % 2 == 0) even.push_back(5000 + 3 * (int64_t)i);
    }
    auto s = Searcher::build(ctx, rows, (int)dim, Metric::Cosine);
    const Moments mo = s->moments({1}, true);
    EXPECT(mo.n == participating && mo.sums == sums && mo.matrix.size() == cov.size());
    EXPECT(std::memcmp(mo.matrix.data(), cov.data(), cov.size() * sizeof(double)) == 0);
    const pcv_moment_stats st = s->last_moment_stats();
    EXPECT(st.rows == (int64_t)n && st.participating == participating && st.row_ranges >= 1 && st.syrk_ms > 0.0f);
    const Moments only = s->moments({1}, false, false);
    EXPECT(only.sums == sums && only.matrix.empty() && s->last_moment_stats().row_ranges == 0);
    const Moments none = s->moments({}, true);  // an empty filter selects nothing
    EXPECT(none.n == 0 && none.sums == std::vector<int64_t>(dim, 0));

    const Projection pr = s->project({1}, axes, m, &offsets);
    EXPECT(pr.coords.size() == coords.size() && pr.ids.size() == n);
    EXPECT(std::memcmp(pr.coords.data(), coords.data(), coords.size() * sizeof(float)) == 0);
    for (size_t i = 0; i < pr.ids.size(); ++i) EXPECT(pr.ids[i] == 5000 + 3 * (int64_t)i);
    EXPECT(s->last_project_stats().axes == (int32_t)m && s->last_project_stats().rows == (int64_t)n);
    EXPECT(s->project({}, axes, m).ids.empty());

    const Eigen eg = symmetric_eigen(cov, dim);
    const PrincipalAxes pa = s->principal_axes({1}, 2);
    EXPECT(pa.n == participating && pa.axes.size() == 2 * dim && pa.offsets.size() == 2 && pa.variance.size() == 2);
    for (size_t j = 0; j < 2; ++j) {
        EXPECT(eg.values[j] >= eg.values[j + 1]);
        EXPECT(pa.variance[j] == eg.values[j] / ((double)participating * (double)participating));
        for (size_t d = 0; d < dim; ++d) EXPECT(pa.axes[j * dim + d] == (float)eg.vectors[j * dim + d]);
    }

    SearcherView v = s->view(even);
    const Moments vm = v.moments({1}, false);
    EXPECT(vm.n > 0 && vm.n <= (int64_t)even.size() && v.last_moment_stats().rows == (int64_t)even.size());
    const Projection vp = v.project({1}, axes, m, &offsets);
    EXPECT(vp.ids == even);
    for (size_t i = 0; i < even.size(); ++i) EXPECT(std::memcmp(&vp.coords[i * m], &coords[2 * i * m], m * sizeof(float)) == 0);
    if (failures == 0) std::printf("moments_mirror_test: ok\n");
    return failures == 0 ? 0 : 1;
}
