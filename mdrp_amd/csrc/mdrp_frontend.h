// mdrp_frontend.h — the device front end: from a matcher's output (keypoint tables, index pairs) and two depth maps to the
// estimators' padded float64 correspondences, without a trip through the host.
//
// The reference's callers prepare the estimator's input in four NumPy lines (make_pair.py:96-106, make_video.py:265-275): gather the
// matched keypoints, read each keypoint's depth at the truncated pixel, drop a correspondence whose depths are both infinite.  The same
// per-row rule lives here once, as host + device inline functions (fe_pixel, fe_keep): k_gather applies it on the device,
// tests/hostmath/frontend_host.cpp pins it on the CPU against mdrp_amd/frontend.py, the NumPy statement of the same definition.
// k_gather_images is the same front end for a batch held per image (mdrp_image_pairs: one keypoint table and one depth map per image, pairs as
// image indices); its per-image rules (fe_image_valid, fe_clamp_extent, the table offsets) are pinned by tests/hostmath/image_pairs_host.cpp.
// Like mdrp_math.h, the header compiles with a plain host C++ compiler (the kernels are left out there); that build is test scaffolding.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef MDRP_HD
#if defined(__HIPCC__)
#define MDRP_HD __host__ __device__ __forceinline__
#else
#define MDRP_HD inline
#endif
#endif

namespace mdrp {

constexpr int FE_FILTER_BOTH_INF = 0; // == MDRP_FILTER_BOTH_INF: drop a row iff both depths are infinite (the reference scripts' rule)
constexpr int FE_FILTER_FINITE = 1;   // == MDRP_FILTER_FINITE: keep a row only when both depths are finite

// Index range of a match row: -1 (or any negative index) is padding, an index past its keypoint table is dropped as well.
MDRP_HD bool fe_row_valid(int i, int j, int k1, int k2) { return i >= 0 && j >= 0 && i < k1 && j < k2; }

// Pixel of a keypoint in a w x h map: the coordinate truncated toward zero, as astype(int) does in range.  The range test is made on the
// floating value (widened to double, which is exact for float and for w, h): x in (-1, w), y in (-1, h).  -0.5 is pixel 0 and w - 0.001
// is pixel w - 1; -1, w, NaN and +-inf fail (every comparison with a NaN is false), so the conversion below never sees a value outside int.
template <typename T> MDRP_HD bool fe_pixel(T x, T y, int w, int h, int &xi, int &yi) {
    const double xd = (double)x, yd = (double)y;
    const bool in = xd > -1.0 && xd < (double)w && yd > -1.0 && yd < (double)h;
    xi = in ? (int)xd : 0;
    yi = in ? (int)yd : 0;
    return in;
}

// bit patterns, not isinf / isfinite: the same answer on host and device whatever the fast-math settings of the build
MDRP_HD bool fe_isinf(double d) {
    union { double f; uint64_t u; } v;
    v.f = d;
    return (v.u & 0x7fffffffffffffffull) == 0x7ff0000000000000ull;
}
MDRP_HD bool fe_isfinite(double d) {
    union { double f; uint64_t u; } v;
    v.f = d;
    return (v.u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// The depth filter.  "both_inf" keeps a NaN depth and a one-sided infinity, exactly as the scripts do.
MDRP_HD bool fe_keep(double d1, double d2, int filter) {
    if (filter == FE_FILTER_FINITE) return fe_isfinite(d1) && fe_isfinite(d2);
    return !(fe_isinf(d1) && fe_isinf(d2));
}

// ---- per-image tables (mdrp_image_pairs): a pair is two indices into one set of images
// An image index outside [0, n_images) drops every row of its pair; nothing is read through it.
MDRP_HD bool fe_image_valid(int a, int n_images) { return a >= 0 && a < n_images; }

// A per-image extent (kp_count, the h and w of size) against the allocated one: clamped to [0, max], so that no valid index leaves the table.
MDRP_HD int fe_clamp_extent(int v, int max) { return v < 0 ? 0 : (v > max ? max : v); }

// Offsets of image a's tables in elements, from the image index and in size_t: [I][k_max][2] keypoints, [I][h_max][w_max] depths.
MDRP_HD size_t fe_kp_offset(int a, int k_max, int i) { return 2 * ((size_t)a * (size_t)k_max + (size_t)i); }
MDRP_HD size_t fe_depth_offset(int a, int h_max, int w_max, int yi, int xi) {
    return ((size_t)a * (size_t)h_max + (size_t)yi) * (size_t)w_max + (size_t)xi; // the row stride is w_max, whatever the valid width
}

#if defined(__HIPCC__)

constexpr int FE_THREADS = 256; // one workgroup per pair, four wavefronts

// One workgroup per pair walks the match rows in tiles of FE_THREADS.  Kept rows go to consecutive slots IN MATCH ORDER (the sampler
// indexes correspondences by position: the estimate must see them in the order the NumPy route produces): a row's slot is the running
// base of the tiles before it + the kept rows of the wavefronts before its own (a 4-entry LDS table) + the kept rows of the lower lanes
// of its wavefront (ballot + popcount).  Behind the kept rows the buffers get the filler of poselib._stack (x = 0, d = 1).
template <typename KpT, typename DepthT>
__global__ __launch_bounds__(FE_THREADS) void k_gather(const KpT *__restrict__ kp1, const KpT *__restrict__ kp2, int k1, int k2,
                                                       const int32_t *__restrict__ matches, int m_max, const DepthT *__restrict__ depth1,
                                                       const DepthT *__restrict__ depth2, int h1, int w1, int h2, int w2,
                                                       const double *__restrict__ center1, const double *__restrict__ center2, int filter,
                                                       double *__restrict__ x1, double *__restrict__ x2, double *__restrict__ d1,
                                                       double *__restrict__ d2, int32_t *__restrict__ slot, int32_t *__restrict__ n_out) {
    __shared__ int s_wave[FE_THREADS / 64];
    const size_t b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row0 = b * (size_t)m_max;
    const double c1x = center1 ? center1[2 * b] : 0.0, c1y = center1 ? center1[2 * b + 1] : 0.0;
    const double c2x = center2 ? center2[2 * b] : 0.0, c2y = center2 ? center2[2 * b + 1] : 0.0;
    int base = 0;
    for (int m0 = 0; m0 < m_max; m0 += FE_THREADS) {
        const int m = m0 + (int)threadIdx.x;
        bool keep = false;
        double p1x = 0.0, p1y = 0.0, p2x = 0.0, p2y = 0.0, e1 = 0.0, e2 = 0.0;
        if (m < m_max) {
            const int i = matches[2 * (row0 + m)], j = matches[2 * (row0 + m) + 1];
            if (fe_row_valid(i, j, k1, k2)) {
                const KpT *q1 = kp1 + 2 * (b * (size_t)k1 + (size_t)i), *q2 = kp2 + 2 * (b * (size_t)k2 + (size_t)j);
                const KpT a1x = q1[0], a1y = q1[1], a2x = q2[0], a2y = q2[1];
                int xi1, yi1, xi2, yi2;
                const bool in1 = fe_pixel(a1x, a1y, w1, h1, xi1, yi1), in2 = fe_pixel(a2x, a2y, w2, h2, xi2, yi2);
                if (in1 && in2) {
                    e1 = (double)depth1[(b * (size_t)h1 + (size_t)yi1) * (size_t)w1 + (size_t)xi1];
                    e2 = (double)depth2[(b * (size_t)h2 + (size_t)yi2) * (size_t)w2 + (size_t)xi2];
                    keep = fe_keep(e1, e2, filter);
                    p1x = (double)a1x - c1x; p1y = (double)a1y - c1y;
                    p2x = (double)a2x - c2x; p2y = (double)a2y - c2y;
                }
            }
        }
        const unsigned long long ball = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(ball);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < FE_THREADS / 64; ++w) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (m < m_max) {
            const int s = base + before + __popcll(ball & ((1ull << lane) - 1ull));
            slot[row0 + m] = keep ? s : -1;
            if (keep) { // s < m_max: at most one slot per row
                const size_t at = row0 + (size_t)s;
                x1[2 * at] = p1x; x1[2 * at + 1] = p1y;
                x2[2 * at] = p2x; x2[2 * at + 1] = p2y;
                d1[at] = e1; d2[at] = e2;
            }
        }
        base += total;
        __syncthreads(); // s_wave is rewritten by the next tile
    }
    for (int s = base + (int)threadIdx.x; s < m_max; s += FE_THREADS) {
        const size_t at = row0 + (size_t)s;
        x1[2 * at] = 0.0; x1[2 * at + 1] = 0.0;
        x2[2 * at] = 0.0; x2[2 * at + 1] = 0.0;
        d1[at] = 1.0; d2[at] = 1.0;
    }
    if (threadIdx.x == 0) n_out[b] = base;
}

// k_gather for a batch described the way its producer holds it: keypoints, depth maps, sizes, counts and centres exist once per IMAGE
// and pair b is (a, c) = pairs[b], two indices into them.  Rules 1-5 and the ordered compaction are k_gather's; the tables are addressed
// from the image index (fe_kp_offset, fe_depth_offset), image a's extents are its own, clamped to the allocation (fe_clamp_extent).  A
// pair with an index outside [0, n_images) keeps no row: it walks the same tiles with keep = false (every barrier is reached, slot = -1
// and the filler are written) and loads nothing from the tables, not even its match rows.
template <typename KpT, typename DepthT>
__global__ __launch_bounds__(FE_THREADS) void k_gather_images(const KpT *__restrict__ kp, const int32_t *__restrict__ kp_count, int k_max,
                                                              const DepthT *__restrict__ depth, const int32_t *__restrict__ size, int h_max,
                                                              int w_max, const double *__restrict__ center, int n_images,
                                                              const int32_t *__restrict__ pairs, const int32_t *__restrict__ matches, int m_max,
                                                              int filter, double *__restrict__ x1, double *__restrict__ x2,
                                                              double *__restrict__ d1, double *__restrict__ d2, int32_t *__restrict__ slot,
                                                              int32_t *__restrict__ n_out) {
    __shared__ int s_wave[FE_THREADS / 64];
    const size_t b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row0 = b * (size_t)m_max;
    const int a = pairs[2 * b], c = pairs[2 * b + 1];
    const bool pair_ok = fe_image_valid(a, n_images) && fe_image_valid(c, n_images); // uniform over the workgroup
    int k1 = 0, k2 = 0, h1 = 0, w1 = 0, h2 = 0, w2 = 0;
    double c1x = 0.0, c1y = 0.0, c2x = 0.0, c2y = 0.0;
    if (pair_ok) {
        k1 = kp_count ? fe_clamp_extent(kp_count[a], k_max) : k_max;
        k2 = kp_count ? fe_clamp_extent(kp_count[c], k_max) : k_max;
        h1 = size ? fe_clamp_extent(size[2 * (size_t)a], h_max) : h_max;
        w1 = size ? fe_clamp_extent(size[2 * (size_t)a + 1], w_max) : w_max;
        h2 = size ? fe_clamp_extent(size[2 * (size_t)c], h_max) : h_max;
        w2 = size ? fe_clamp_extent(size[2 * (size_t)c + 1], w_max) : w_max;
        if (center) {
            c1x = center[2 * (size_t)a]; c1y = center[2 * (size_t)a + 1];
            c2x = center[2 * (size_t)c]; c2y = center[2 * (size_t)c + 1];
        }
    }
    int base = 0;
    for (int m0 = 0; m0 < m_max; m0 += FE_THREADS) {
        const int m = m0 + (int)threadIdx.x;
        bool keep = false;
        double p1x = 0.0, p1y = 0.0, p2x = 0.0, p2y = 0.0, e1 = 0.0, e2 = 0.0;
        if (pair_ok && m < m_max) {
            const int i = matches[2 * (row0 + m)], j = matches[2 * (row0 + m) + 1];
            if (fe_row_valid(i, j, k1, k2)) { // i < k1 <= k_max, j < k2 <= k_max
                const KpT *q1 = kp + fe_kp_offset(a, k_max, i), *q2 = kp + fe_kp_offset(c, k_max, j);
                const KpT a1x = q1[0], a1y = q1[1], a2x = q2[0], a2y = q2[1];
                int xi1, yi1, xi2, yi2;
                const bool in1 = fe_pixel(a1x, a1y, w1, h1, xi1, yi1), in2 = fe_pixel(a2x, a2y, w2, h2, xi2, yi2);
                if (in1 && in2) { // yi < h <= h_max, xi < w <= w_max
                    e1 = (double)depth[fe_depth_offset(a, h_max, w_max, yi1, xi1)];
                    e2 = (double)depth[fe_depth_offset(c, h_max, w_max, yi2, xi2)];
                    keep = fe_keep(e1, e2, filter);
                    p1x = (double)a1x - c1x; p1y = (double)a1y - c1y;
                    p2x = (double)a2x - c2x; p2y = (double)a2y - c2y;
                }
            }
        }
        const unsigned long long ball = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(ball);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < FE_THREADS / 64; ++w) {
            const int cnt = s_wave[w];
            before += w < wave ? cnt : 0;
            total += cnt;
        }
        if (m < m_max) {
            const int s = base + before + __popcll(ball & ((1ull << lane) - 1ull));
            slot[row0 + m] = keep ? s : -1;
            if (keep) { // s < m_max: at most one slot per row
                const size_t at = row0 + (size_t)s;
                x1[2 * at] = p1x; x1[2 * at + 1] = p1y;
                x2[2 * at] = p2x; x2[2 * at + 1] = p2y;
                d1[at] = e1; d2[at] = e2;
            }
        }
        base += total;
        __syncthreads(); // s_wave is rewritten by the next tile
    }
    for (int s = base + (int)threadIdx.x; s < m_max; s += FE_THREADS) {
        const size_t at = row0 + (size_t)s;
        x1[2 * at] = 0.0; x1[2 * at + 1] = 0.0;
        x2[2 * at] = 0.0; x2[2 * at + 1] = 0.0;
        d1[at] = 1.0; d2[at] = 1.0;
    }
    if (threadIdx.x == 0) n_out[b] = base;
}

// the estimator's inlier mask (one byte per kept correspondence, by slot) back onto the match rows: dropped rows are 0
__global__ __launch_bounds__(FE_THREADS) void k_match_mask(const int32_t *__restrict__ slot, const uint8_t *__restrict__ mask, int m_max, size_t rows,
                                                           uint8_t *__restrict__ match_mask) {
    const size_t at = (size_t)blockIdx.x * FE_THREADS + threadIdx.x;
    if (at >= rows) return;
    const int s = slot[at];
    match_mask[at] = s >= 0 ? mask[(at / (size_t)m_max) * (size_t)m_max + (size_t)s] : (uint8_t)0;
}

#endif // __HIPCC__

} // namespace mdrp
