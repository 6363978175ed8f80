// Host build of the front end without depth maps (mdrp_amd/csrc/mdrp_frontend.h: fe_row_valid, fe_point_row, fe_image_valid, fe_clamp_extent,
// fe_kp_offset — what k_gather_points / k_gather_points_images apply per row) for tests/test_classic_frontend_host.py: the rows of a batch walked in
// match order on the CPU, plain C entry points over arrays, no GPU.
//   g++ -O2 -std=c++17 -fPIC -shared points_host.cpp -o libpoints_host.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DPOINTS_HOST_MAIN points_host.cpp -o points_host_san   (stand-alone)
#include "../../mdrp_amd/csrc/mdrp_frontend.h"

#include <cstdio>
#include <limits>
#include <vector>

using namespace mdrp;

namespace {

// the ordered compaction of one pair, sequentially: rows(m, r) as the device functors define it
template <typename Rows> void gather_pair(const Rows &rows, size_t b, int m_max, double *x1, double *x2, int32_t *slot, int32_t *n_out) {
    const size_t row0 = b * (size_t)m_max;
    int s = 0;
    for (int m = 0; m < m_max; ++m) {
        FeRow r;
        const bool keep = rows(m, r);
        slot[row0 + m] = keep ? s : -1;
        if (!keep) continue;
        const size_t at = row0 + (size_t)s++;
        x1[2 * at] = r.p1x; x1[2 * at + 1] = r.p1y;
        x2[2 * at] = r.p2x; x2[2 * at + 1] = r.p2y;
    }
    for (int t = s; t < m_max; ++t) {
        const size_t at = row0 + (size_t)t;
        x1[2 * at] = x1[2 * at + 1] = x2[2 * at] = x2[2 * at + 1] = 0.0;
    }
    n_out[b] = s;
}

template <typename KpT>
void gather_points(const KpT *kp1, const KpT *kp2, int k1, int k2, const int32_t *matches, int m_max, const double *center1, const double *center2, int batch,
                   double *x1, double *x2, int32_t *slot, int32_t *n_out) {
    for (size_t b = 0; b < (size_t)batch; ++b) {
        const size_t row0 = b * (size_t)m_max;
        const double c1x = center1 ? center1[2 * b] : 0.0, c1y = center1 ? center1[2 * b + 1] : 0.0;
        const double c2x = center2 ? center2[2 * b] : 0.0, c2y = center2 ? center2[2 * b + 1] : 0.0;
        gather_pair([&](int m, FeRow &r) {
            const int i = matches[2 * (row0 + m)], j = matches[2 * (row0 + m) + 1];
            if (!fe_row_valid(i, j, k1, k2)) return false;
            return fe_point_row(kp1 + 2 * (b * (size_t)k1 + (size_t)i), kp2 + 2 * (b * (size_t)k2 + (size_t)j), c1x, c1y, c2x, c2y, r);
        }, b, m_max, x1, x2, slot, n_out);
    }
}

template <typename KpT>
void gather_point_images(const KpT *kp, const int32_t *kp_count, int k_max, const double *center, int n_images, const int32_t *pairs, const int32_t *matches,
                         int m_max, int batch, double *x1, double *x2, int32_t *slot, int32_t *n_out) {
    for (size_t b = 0; b < (size_t)batch; ++b) {
        const size_t row0 = b * (size_t)m_max;
        const int a = pairs[2 * b], c = pairs[2 * b + 1];
        const bool pair_ok = fe_image_valid(a, n_images) && fe_image_valid(c, n_images);
        int k1 = 0, k2 = 0;
        double c1x = 0.0, c1y = 0.0, c2x = 0.0, c2y = 0.0;
        if (pair_ok) {
            k1 = kp_count ? fe_clamp_extent(kp_count[a], k_max) : k_max;
            k2 = kp_count ? fe_clamp_extent(kp_count[c], k_max) : k_max;
            if (center) {
                c1x = center[2 * (size_t)a]; c1y = center[2 * (size_t)a + 1];
                c2x = center[2 * (size_t)c]; c2y = center[2 * (size_t)c + 1];
            }
        }
        gather_pair([&](int m, FeRow &r) {
            if (!pair_ok) return false;
            const int i = matches[2 * (row0 + m)], j = matches[2 * (row0 + m) + 1];
            if (!fe_row_valid(i, j, k1, k2)) return false;
            return fe_point_row(kp + fe_kp_offset(a, k_max, i), kp + fe_kp_offset(c, k_max, j), c1x, c1y, c2x, c2y, r);
        }, b, m_max, x1, x2, slot, n_out);
    }
}

} // namespace

extern "C" {

void ph_gather_points_f32(const float *kp1, const float *kp2, int k1, int k2, const int32_t *matches, int m_max, const double *center1, const double *center2,
                          int batch, double *x1, double *x2, int32_t *slot, int32_t *n_out) {
    gather_points(kp1, kp2, k1, k2, matches, m_max, center1, center2, batch, x1, x2, slot, n_out);
}
void ph_gather_points_f64(const double *kp1, const double *kp2, int k1, int k2, const int32_t *matches, int m_max, const double *center1, const double *center2,
                          int batch, double *x1, double *x2, int32_t *slot, int32_t *n_out) {
    gather_points(kp1, kp2, k1, k2, matches, m_max, center1, center2, batch, x1, x2, slot, n_out);
}
void ph_gather_point_images_f32(const float *kp, const int32_t *kp_count, int k_max, const double *center, int n_images, const int32_t *pairs,
                                const int32_t *matches, int m_max, int batch, double *x1, double *x2, int32_t *slot, int32_t *n_out) {
    gather_point_images(kp, kp_count, k_max, center, n_images, pairs, matches, m_max, batch, x1, x2, slot, n_out);
}
void ph_gather_point_images_f64(const double *kp, const int32_t *kp_count, int k_max, const double *center, int n_images, const int32_t *pairs,
                                const int32_t *matches, int m_max, int batch, double *x1, double *x2, int32_t *slot, int32_t *n_out) {
    gather_point_images(kp, kp_count, k_max, center, n_images, pairs, matches, m_max, batch, x1, x2, slot, n_out);
}
}

#ifdef POINTS_HOST_MAIN
// Stand-alone: tables allocated to their exact size, every kind of row that must not be read through (padding, indices past the table and past the
// clamped count, an image index out of range) next to rows that are kept.  Under -fsanitize=address,undefined a read past a table ends the program.
int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const int I = 2, K = 3, M = 8, B = 4;
    std::vector<float> kp = {1, 2, 3, 4, nan, 5, /* image 1 */ 6, 7, 8, -inf, 9, 10};
    std::vector<int32_t> count = {K + 5, 2};             // image 0: clamped to K; image 1: its third keypoint is not valid
    std::vector<double> center = {0.5, 0.25, 1.0, 2.0};
    std::vector<int32_t> pairs = {0, 1, 1, 1, 0, I, -1, 0};
    const int32_t row[M][2] = {{0, 0}, {-1, 0}, {2, 0}, {1, 1}, {1, 2}, {K, 0}, {0, -7}, {1, 0}};
    std::vector<int32_t> matches;
    for (int b = 0; b < B; ++b)
        for (int m = 0; m < M; ++m) { matches.push_back(row[m][0]); matches.push_back(row[m][1]); }
    std::vector<double> x1((size_t)B * M * 2, -1.0), x2((size_t)B * M * 2, -1.0);
    std::vector<int32_t> slot((size_t)B * M, -2), n(B, -2);
    ph_gather_point_images_f32(kp.data(), count.data(), K, center.data(), I, pairs.data(), matches.data(), M, B, x1.data(), x2.data(), slot.data(), n.data());
    // pair (0, 1): rows 0 and 7 are kept (row 2: NaN, row 3: -inf, row 4: past image 1's count); pair (1, 1): row 0 alone (row 7 meets the -inf); the other two are empty
    const int want_n[B] = {2, 1, 0, 0};
    int bad = 0;
    for (int b = 0; b < B; ++b) bad += n[b] != want_n[b];
    bad += slot[0] != 0 || slot[7] != 1 || slot[2] != -1 || slot[3] != -1 || slot[4] != -1 || slot[5] != -1;
    bad += x1[0] != 0.5 || x1[1] != 1.75 || x2[0] != 5.0 || x2[1] != 5.0 || x1[2] != 2.5 || x2[2] != 5.0;
    for (int m = 0; m < M; ++m) bad += slot[(size_t)2 * M + m] != -1 || slot[(size_t)3 * M + m] != -1;
    // the per-pair form on two tables of K rows each
    std::vector<float> t1(kp.begin(), kp.begin() + 2 * K), t2(kp.begin() + 2 * K, kp.end());
    std::vector<int32_t> one(matches.begin(), matches.begin() + 2 * M);
    ph_gather_points_f32(t1.data(), t2.data(), K, K, one.data(), M, nullptr, nullptr, 1, x1.data(), x2.data(), slot.data(), n.data());
    bad += n[0] != 3 || slot[0] != 0 || slot[4] != 1 || slot[7] != 2 || slot[3] != -1; // (row 4 reaches image 1's third keypoint here)
    std::printf("points_host: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
