// moments_host.cpp — the host-only entry points of "Corpus moments and principal axes" (DESIGN.md §4): the 128-bit finish of
// pcv_searcher_moments and the Jacobi eigen-solver.  Neither needs a context or a GPU.
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "common.h"

namespace pcv {
namespace {

// (double)v * 2^-64, v an exact integer: one rounding, to nearest even; the power of two is exact (|v| < 2^127, so no result is
// subnormal or infinite).
double int128_to_scaled_double(__int128 v) {
    const bool neg = v < 0;
    unsigned __int128 u = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
    if (u == 0) return 0.0;
    int bits = 0;
    for (unsigned __int128 w = u; w != 0; w >>= 1) ++bits;
    int sh = 0;
    if (bits > 53) {
        sh = bits - 53;
        const unsigned __int128 rem = u & (((unsigned __int128)1 << sh) - 1), half = (unsigned __int128)1 << (sh - 1);
        u >>= sh;
        if (rem > half || (rem == half && (u & 1))) ++u;  // (2^53 at most: still exact below)
    }
    const double d = std::ldexp((double)(uint64_t)u, sh - 64);
    return neg ? -d : d;
}

// Cyclic Jacobi (Rutishauser's form of the rotation): A is rotated in place, V accumulates the rotations by rows — row i of V is
// the i-th eigenvector.  Rows p and q of A and of V are contiguous; the columns of A are mirrored from them.
void jacobi(std::vector<double>& A, std::vector<double>& V, int n) {
    double total = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) total += A[(size_t)i * n + j] * A[(size_t)i * n + j];
    const double stop = std::sqrt(total) * 0x1p-56;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) off += A[(size_t)i * n + j] * A[(size_t)i * n + j];
        if (!(std::sqrt(2.0 * off) > stop)) break;
        for (int p = 0; p < n - 1; ++p) {
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[(size_t)p * n + q];
                if (apq == 0.0) continue;
                const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
                // negligible beside both diagonal entries: annihilate without a rotation
                if (sweep >= 3 && std::fabs(app) + 128.0 * std::fabs(apq) == std::fabs(app) && std::fabs(aqq) + 128.0 * std::fabs(apq) == std::fabs(aqq)) {
                    A[(size_t)p * n + q] = A[(size_t)q * n + p] = 0.0;
                    continue;
                }
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c, tau = sn / (1.0 + c);
                double* ap = &A[(size_t)p * n];
                double* aq = &A[(size_t)q * n];
                for (int k = 0; k < n; ++k) {
                    const double g = ap[k], h = aq[k];
                    ap[k] = g - sn * (h + g * tau);
                    aq[k] = h + sn * (g - h * tau);
                }
                ap[p] = app - t * apq;
                aq[q] = aqq + t * apq;
                ap[q] = aq[p] = 0.0;
                for (int k = 0; k < n; ++k) {  // the columns, from the rows
                    if (k == p || k == q) continue;
                    A[(size_t)k * n + p] = ap[k];
                    A[(size_t)k * n + q] = aq[k];
                }
                double* vp = &V[(size_t)p * n];
                double* vq = &V[(size_t)q * n];
                for (int k = 0; k < n; ++k) {
                    const double g = vp[k], h = vq[k];
                    vp[k] = g - sn * (h + g * tau);
                    vq[k] = h + sn * (g - h * tau);
                }
            }
        }
    }
}

}  // namespace
}  // namespace pcv

using namespace pcv;

extern "C" {

pcv_status pcv_moments_finish(const int64_t* hh, const int64_t* hl, const int64_t* ll, const int64_t* sums, int64_t n, int dim, int centered,
                              double* out_matrix) {
    return guarded([&] {
        PCV_REQUIRE(hh != nullptr && hl != nullptr && ll != nullptr && out_matrix != nullptr, "moments_finish: a matrix is NULL");
        PCV_REQUIRE(dim >= 1, "moments_finish: dim %d", dim);
        PCV_REQUIRE(n >= 0 && n <= ((int64_t)1 << 30), "moments_finish: n %lld outside [0, 2^30]", (long long)n);
        PCV_REQUIRE(!centered || sums != nullptr, "moments_finish: sums is NULL with centered set");
        const size_t D = (size_t)dim;
        for (size_t d = 0; d < D; ++d) {
            for (size_t e = d; e < D; ++e) {
                __int128 c = (__int128)hh[d * D + e] * ((__int128)1 << 32) + ((__int128)hl[d * D + e] + (__int128)hl[e * D + d]) * ((__int128)1 << 16) +
                             (__int128)ll[d * D + e];
                if (centered) c = (__int128)n * c - (__int128)sums[d] * (__int128)sums[e];
                out_matrix[d * D + e] = out_matrix[e * D + d] = int128_to_scaled_double(c);
            }
        }
    });
}

pcv_status pcv_symmetric_eigen(const double* a, int n, double* out_values, double* out_vectors) {
    return guarded([&] {
        PCV_REQUIRE(a != nullptr && out_values != nullptr && out_vectors != nullptr, "symmetric_eigen: NULL argument");
        PCV_REQUIRE(n >= 1 && n <= 2048, "symmetric_eigen: n %d outside [1,2048]", n);
        const size_t N = (size_t)n;
        std::vector<double> A(N * N), V(N * N, 0.0);
        for (size_t i = 0; i < N; ++i) {
            for (size_t j = i; j < N; ++j) {
                const double x = a[i * N + j];
                PCV_REQUIRE(std::isfinite(x), "symmetric_eigen: a[%zu][%zu] is not finite", i, j);
                A[i * N + j] = A[j * N + i] = x;
            }
            V[i * N + i] = 1.0;
        }
        jacobi(A, V, n);
        std::vector<int> order(N);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return A[(size_t)x * N + x] > A[(size_t)y * N + y]; });
        for (size_t i = 0; i < N; ++i) {
            const double* v = &V[(size_t)order[i] * N];
            double norm2 = 0.0, big = 0.0;
            size_t at = 0;
            for (size_t k = 0; k < N; ++k) {
                norm2 += v[k] * v[k];
                if (std::fabs(v[k]) > big) big = std::fabs(v[k]), at = k;
            }
            const double f = (v[at] < 0.0 ? -1.0 : 1.0) / std::sqrt(norm2);
            out_values[i] = A[(size_t)order[i] * N + order[i]];
            for (size_t k = 0; k < N; ++k) out_vectors[i * N + k] = v[k] * f;
        }
    });
}

}  // extern "C"
