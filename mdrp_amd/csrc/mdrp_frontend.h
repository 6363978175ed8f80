// mdrp_frontend.h — the device front end: from a matcher's output (keypoint tables, index pairs) and two depth maps to the
// estimators' padded float64 correspondences, without a trip through the host.
//
// The reference's callers prepare the estimator's input in four NumPy lines (make_pair.py:96-106, make_video.py:265-275): gather the
// matched keypoints, read each keypoint's depth at the truncated pixel, drop a correspondence whose depths are both infinite.  The same
// per-row rule lives here once, as host + device inline functions (fe_pixel, fe_keep): k_gather applies it on the device,
// tests/hostmath/frontend_host.cpp pins it on the CPU against mdrp_amd/frontend.py, the NumPy statement of the same definition.
// k_gather_images is the same front end for a batch held per image (mdrp_image_pairs: one keypoint table and one depth map per image, pairs as
// image indices); its per-image rules (fe_image_valid, fe_clamp_extent, the table offsets) are pinned by tests/hostmath/image_pairs_host.cpp.
// k_gather_ranked / k_gather_images_ranked are the same two front ends with one score per match row: a kept row goes to its RANK
// among the kept rows of its pair, so that the progressive sampler (mdrp_prosac.h) runs on the gathered buffers as they are.
// k_gather_points* are the four again without depth maps, for the 5- / 6- / 7-point baselines: the row rule is fe_point_row
// (tests/hostmath/points_host.cpp), the compactions are shared through the row functors' HAS_DEPTH.
// Like mdrp_math.h, the header compiles with a plain host C++ compiler (the kernels are left out there); that build is test scaffolding.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include "mdrp_prosac.h" // rank_key, rank_count: the ranked front end ranks as k_rank does
#endif

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

// Rules 1-4 for one match row, once for every kernel of the front end: what a kept row gathers, and whether it is kept.
struct FeRow {
    double p1x = 0.0, p1y = 0.0, p2x = 0.0, p2y = 0.0, e1 = 0.0, e2 = 0.0; // centred keypoints, depths
};

// ---- the front end without depth maps (include/mdrp_classic_frontend.h): the 5- / 6- / 7-point baselines take correspondences alone
// A row of valid indices is kept iff its four coordinates are finite: there is no map to be inside of and no depth to filter on.
template <typename KpT> MDRP_HD bool fe_point_row(const KpT *q1, const KpT *q2, double c1x, double c1y, double c2x, double c2y, FeRow &r) {
    const double a1x = (double)q1[0], a1y = (double)q1[1], a2x = (double)q2[0], a2y = (double)q2[1];
    r.p1x = a1x - c1x; r.p1y = a1y - c1y;
    r.p2x = a2x - c2x; r.p2y = a2y - c2y;
    return fe_isfinite(a1x) && fe_isfinite(a1y) && fe_isfinite(a2x) && fe_isfinite(a2y);
}

#if defined(__HIPCC__)

constexpr int FE_THREADS = 256; // one workgroup per pair, four wavefronts

// the rows of pair b of an mdrp_matches batch
template <typename KpT, typename DepthT> struct FeMatchRows {
    static constexpr bool HAS_DEPTH = true; // the row carries depths: fe_gather_ordered / fe_gather_ranked write d1, d2
    const KpT *kp1, *kp2;
    int k1, k2;
    const int32_t *matches;
    const DepthT *depth1, *depth2;
    int h1, w1, h2, w2;
    double c1x, c1y, c2x, c2y;
    int filter;
    size_t b, row0;
    __device__ __forceinline__ bool operator()(int m, FeRow &r) const { // m in [0, m_max)
        bool keep = false;
        const int i = matches[2 * (row0 + m)], j = matches[2 * (row0 + m) + 1];
        if (fe_row_valid(i, j, k1, k2)) {
            const KpT *q1 = kp1 + 2 * (b * (size_t)k1 + (size_t)i), *q2 = kp2 + 2 * (b * (size_t)k2 + (size_t)j);
            const KpT a1x = q1[0], a1y = q1[1], a2x = q2[0], a2y = q2[1];
            int xi1, yi1, xi2, yi2;
            const bool in1 = fe_pixel(a1x, a1y, w1, h1, xi1, yi1), in2 = fe_pixel(a2x, a2y, w2, h2, xi2, yi2);
            if (in1 && in2) {
                r.e1 = (double)depth1[(b * (size_t)h1 + (size_t)yi1) * (size_t)w1 + (size_t)xi1];
                r.e2 = (double)depth2[(b * (size_t)h2 + (size_t)yi2) * (size_t)w2 + (size_t)xi2];
                keep = fe_keep(r.e1, r.e2, filter);
                r.p1x = (double)a1x - c1x; r.p1y = (double)a1y - c1y;
                r.p2x = (double)a2x - c2x; r.p2y = (double)a2y - c2y;
            }
        }
        return keep;
    }
};

// the rows of pair (a, c) of an mdrp_image_pairs batch; a pair with an index outside the image set keeps no row and loads nothing
template <typename KpT, typename DepthT> struct FeImageRows {
    static constexpr bool HAS_DEPTH = true;
    const KpT *kp;
    const DepthT *depth;
    const int32_t *matches;
    int k_max, h_max, w_max, a, c;
    bool pair_ok;
    int k1 = 0, k2 = 0, h1 = 0, w1 = 0, h2 = 0, w2 = 0;
    double c1x = 0.0, c1y = 0.0, c2x = 0.0, c2y = 0.0;
    int filter;
    size_t row0;
    __device__ __forceinline__ FeImageRows(const KpT *kp_, const int32_t *kp_count, int k_max_, const DepthT *depth_, const int32_t *size, int h_max_,
                                           int w_max_, const double *center, int n_images, const int32_t *pairs, const int32_t *matches_, int filter_,
                                           size_t b, size_t row0_)
        : kp(kp_), depth(depth_), matches(matches_), k_max(k_max_), h_max(h_max_), w_max(w_max_), a(pairs[2 * b]), c(pairs[2 * b + 1]),
          pair_ok(fe_image_valid(a, n_images) && fe_image_valid(c, n_images)) /*uniform over the workgroup*/, filter(filter_), row0(row0_) {
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
    }
    __device__ __forceinline__ bool operator()(int m, FeRow &r) const { // m in [0, m_max)
        bool keep = false;
        if (pair_ok) {
            const int i = matches[2 * (row0 + m)], j = matches[2 * (row0 + m) + 1];
            if (fe_row_valid(i, j, k1, k2)) { // i < k1 <= k_max, j < k2 <= k_max
                const KpT *q1 = kp + fe_kp_offset(a, k_max, i), *q2 = kp + fe_kp_offset(c, k_max, j);
                const KpT a1x = q1[0], a1y = q1[1], a2x = q2[0], a2y = q2[1];
                int xi1, yi1, xi2, yi2;
                const bool in1 = fe_pixel(a1x, a1y, w1, h1, xi1, yi1), in2 = fe_pixel(a2x, a2y, w2, h2, xi2, yi2);
                if (in1 && in2) { // yi < h <= h_max, xi < w <= w_max
                    r.e1 = (double)depth[fe_depth_offset(a, h_max, w_max, yi1, xi1)];
                    r.e2 = (double)depth[fe_depth_offset(c, h_max, w_max, yi2, xi2)];
                    keep = fe_keep(r.e1, r.e2, filter);
                    r.p1x = (double)a1x - c1x; r.p1y = (double)a1y - c1y;
                    r.p2x = (double)a2x - c2x; r.p2y = (double)a2y - c2y;
                }
            }
        }
        return keep;
    }
};

// the rows of pair b of an mdrp_point_matches batch: FeMatchRows without the maps
template <typename KpT> struct FePointMatchRows {
    static constexpr bool HAS_DEPTH = false; // no depth buffer is written or read: d1 = d2 = nullptr
    const KpT *kp1, *kp2;
    int k1, k2;
    const int32_t *matches;
    double c1x, c1y, c2x, c2y;
    size_t b, row0;
    __device__ __forceinline__ bool operator()(int m, FeRow &r) const { // m in [0, m_max)
        const int i = matches[2 * (row0 + m)], j = matches[2 * (row0 + m) + 1];
        if (!fe_row_valid(i, j, k1, k2)) return false;
        return fe_point_row(kp1 + 2 * (b * (size_t)k1 + (size_t)i), kp2 + 2 * (b * (size_t)k2 + (size_t)j), c1x, c1y, c2x, c2y, r);
    }
};

// the rows of pair (a, c) of an mdrp_point_image_pairs batch: FeImageRows without the maps
template <typename KpT> struct FePointImageRows {
    static constexpr bool HAS_DEPTH = false;
    const KpT *kp;
    const int32_t *matches;
    int k_max, a, c;
    bool pair_ok;
    int k1 = 0, k2 = 0;
    double c1x = 0.0, c1y = 0.0, c2x = 0.0, c2y = 0.0;
    size_t row0;
    __device__ __forceinline__ FePointImageRows(const KpT *kp_, const int32_t *kp_count, int k_max_, const double *center, int n_images, const int32_t *pairs,
                                                const int32_t *matches_, size_t b, size_t row0_)
        : kp(kp_), matches(matches_), k_max(k_max_), a(pairs[2 * b]), c(pairs[2 * b + 1]),
          pair_ok(fe_image_valid(a, n_images) && fe_image_valid(c, n_images)) /*uniform over the workgroup*/, row0(row0_) {
        if (pair_ok) {
            k1 = kp_count ? fe_clamp_extent(kp_count[a], k_max) : k_max;
            k2 = kp_count ? fe_clamp_extent(kp_count[c], k_max) : k_max;
            if (center) {
                c1x = center[2 * (size_t)a]; c1y = center[2 * (size_t)a + 1];
                c2x = center[2 * (size_t)c]; c2y = center[2 * (size_t)c + 1];
            }
        }
    }
    __device__ __forceinline__ bool operator()(int m, FeRow &r) const { // m in [0, m_max)
        if (!pair_ok) return false; // nothing is loaded, not even the match row
        const int i = matches[2 * (row0 + m)], j = matches[2 * (row0 + m) + 1];
        if (!fe_row_valid(i, j, k1, k2)) return false; // i < k1 <= k_max, j < k2 <= k_max
        return fe_point_row(kp + fe_kp_offset(a, k_max, i), kp + fe_kp_offset(c, k_max, j), c1x, c1y, c2x, c2y, r);
    }
};

// the ordered compaction of k_gather / k_gather_images / k_gather_points / k_gather_points_images for the rows of one pair
// (Rows::HAS_DEPTH false: d1 and d2 are not touched, they may be null)
template <typename Rows>
__device__ __forceinline__ void fe_gather_ordered(const Rows &rows, int *s_wave /*LDS, FE_THREADS / 64*/, size_t b, int m_max, double *__restrict__ x1,
                                                  double *__restrict__ x2, double *__restrict__ d1, double *__restrict__ d2, int32_t *__restrict__ slot,
                                                  int32_t *__restrict__ n_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row0 = b * (size_t)m_max;
    int base = 0;
    for (int m0 = 0; m0 < m_max; m0 += FE_THREADS) {
        const int m = m0 + (int)threadIdx.x;
        bool keep = false;
        FeRow r;
        if (m < m_max) keep = rows(m, r);
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
                x1[2 * at] = r.p1x; x1[2 * at + 1] = r.p1y;
                x2[2 * at] = r.p2x; x2[2 * at + 1] = r.p2y;
                if constexpr (Rows::HAS_DEPTH) { d1[at] = r.e1; d2[at] = r.e2; }
            }
        }
        base += total;
        __syncthreads(); // s_wave is rewritten by the next tile
    }
    for (int s = base + (int)threadIdx.x; s < m_max; s += FE_THREADS) {
        const size_t at = row0 + (size_t)s;
        x1[2 * at] = 0.0; x1[2 * at + 1] = 0.0;
        x2[2 * at] = 0.0; x2[2 * at + 1] = 0.0;
        if constexpr (Rows::HAS_DEPTH) { d1[at] = 1.0; d2[at] = 1.0; }
    }
    if (threadIdx.x == 0) n_out[b] = base;
}

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
    const FeMatchRows<KpT, DepthT> rows{kp1, kp2, k1, k2, matches, depth1, depth2, h1, w1, h2, w2,
                                        center1 ? center1[2 * b] : 0.0, center1 ? center1[2 * b + 1] : 0.0,
                                        center2 ? center2[2 * b] : 0.0, center2 ? center2[2 * b + 1] : 0.0, filter, b, b * (size_t)m_max};
    fe_gather_ordered(rows, s_wave, b, m_max, x1, x2, d1, d2, slot, n_out);
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
    const FeImageRows<KpT, DepthT> rows(kp, kp_count, k_max, depth, size, h_max, w_max, center, n_images, pairs, matches, filter, b, b * (size_t)m_max);
    fe_gather_ordered(rows, s_wave, b, m_max, x1, x2, d1, d2, slot, n_out);
}

// ---- the ranked front end: one score per match row, higher is better; a kept row goes to its rank among the kept rows
constexpr int FE_F32 = 0, FE_F64 = 1; // == MDRP_F32, MDRP_F64: element type of the scores, uniform over the launch
static_assert(FE_THREADS == RANK_THREADS, "the ranked front end counts with k_rank's loop");

__device__ __forceinline__ double fe_score(const void *scores, int score_type, size_t at) { // (float -> double is exact)
    return score_type == FE_F32 ? (double)static_cast<const float *>(scores)[at] : static_cast<const double *>(scores)[at];
}

// Three phases over the rows of pair b, every loop bound a function of m_max alone (each thread reaches each barrier whatever the pair keeps):
//   keys   key[m] = rank_key(score[m]) for a kept row, 0 for a dropped one (below every real key), to the [B][m_max] scratch; n = kept rows
//   rank   rank(m) = #{m' : key[m'] > key[m], or key[m'] == key[m] and m' < m}, by k_rank's counting loop over all m_max keys: a dropped row never
//          counts against a kept one, so this is the stable descending order of the kept rows' scores in match order
//   write  slot[m] = rank(m) or -1; the row rule is evaluated again for a kept row and its record written at its rank (rank < n <= m_max); the
//          filler behind n; n_out
// `keys` is written by one thread and read by the others of the workgroup: it is neither const nor __restrict__, and a barrier stands between.
template <typename Rows>
__device__ __forceinline__ void fe_gather_ranked(const Rows &rows, uint64_t *s_key /*LDS, RANK_TILE*/, int *s_wave /*LDS, FE_THREADS / 64*/, size_t b, int m_max,
                                                 const void *scores, int score_type, uint64_t *keys, double *__restrict__ x1, double *__restrict__ x2,
                                                 double *__restrict__ d1, double *__restrict__ d2, int32_t *__restrict__ slot, int32_t *__restrict__ n_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row0 = b * (size_t)m_max;
    uint64_t *key_b = keys + row0;
    int kept = 0; // of this wavefront
    for (int m0 = 0; m0 < m_max; m0 += FE_THREADS) {
        const int m = m0 + tid;
        bool keep = false;
        if (m < m_max) {
            FeRow r;
            keep = rows(m, r);
            key_b[m] = keep ? rank_key(fe_score(scores, score_type, row0 + m)) : prosac::RANK_KEY_DROPPED;
        }
        kept += __popcll(__ballot(keep));
    }
    if (lane == 0) s_wave[wave] = kept;
    __syncthreads(); // the keys and the counts are the workgroup's from here on
    int n = 0;
#pragma unroll
    for (int w = 0; w < FE_THREADS / 64; ++w) n += s_wave[w];
    for (int base = 0; base < m_max; base += RANK_THREADS * RANK_PER_THREAD) {
        uint64_t key[RANK_PER_THREAD];
        int idx[RANK_PER_THREAD], cnt[RANK_PER_THREAD];
#pragma unroll
        for (int q = 0; q < RANK_PER_THREAD; ++q) {
            idx[q] = base + q * RANK_THREADS + tid;
            key[q] = idx[q] < m_max ? key_b[idx[q]] : prosac::RANK_KEY_DROPPED;
            cnt[q] = 0;
        }
        rank_count(s_key, m_max, tid, [key_b](int j) { return key_b[j]; }, key, idx, cnt);
#pragma unroll
        for (int q = 0; q < RANK_PER_THREAD; ++q) {
            if (idx[q] >= m_max) continue;
            const bool keep = key[q] != prosac::RANK_KEY_DROPPED;
            slot[row0 + idx[q]] = keep ? cnt[q] : -1;
            if (keep) { // cnt < n <= m_max: the kept rows with a better key, or an equal one and an earlier row
                FeRow r;
                rows(idx[q], r);
                const size_t at = row0 + (size_t)cnt[q];
                x1[2 * at] = r.p1x; x1[2 * at + 1] = r.p1y;
                x2[2 * at] = r.p2x; x2[2 * at + 1] = r.p2y;
                if constexpr (Rows::HAS_DEPTH) { d1[at] = r.e1; d2[at] = r.e2; }
            }
        }
    }
    for (int s = n + tid; s < m_max; s += FE_THREADS) {
        const size_t at = row0 + (size_t)s;
        x1[2 * at] = 0.0; x1[2 * at + 1] = 0.0;
        x2[2 * at] = 0.0; x2[2 * at + 1] = 0.0;
        if constexpr (Rows::HAS_DEPTH) { d1[at] = 1.0; d2[at] = 1.0; }
    }
    if (tid == 0) n_out[b] = n;
}

// k_gather with scores: [B][m_max] float or double (score_type), keys: [B][m_max] scratch
template <typename KpT, typename DepthT>
__global__ __launch_bounds__(FE_THREADS) void k_gather_ranked(const KpT *__restrict__ kp1, const KpT *__restrict__ kp2, int k1, int k2,
                                                              const int32_t *__restrict__ matches, int m_max, const DepthT *__restrict__ depth1,
                                                              const DepthT *__restrict__ depth2, int h1, int w1, int h2, int w2,
                                                              const double *__restrict__ center1, const double *__restrict__ center2, int filter,
                                                              const void *__restrict__ scores, int score_type, uint64_t *keys, double *__restrict__ x1,
                                                              double *__restrict__ x2, double *__restrict__ d1, double *__restrict__ d2,
                                                              int32_t *__restrict__ slot, int32_t *__restrict__ n_out) {
    __shared__ uint64_t s_key[RANK_TILE];
    __shared__ int s_wave[FE_THREADS / 64];
    const size_t b = blockIdx.x;
    const FeMatchRows<KpT, DepthT> rows{kp1, kp2, k1, k2, matches, depth1, depth2, h1, w1, h2, w2,
                                        center1 ? center1[2 * b] : 0.0, center1 ? center1[2 * b + 1] : 0.0,
                                        center2 ? center2[2 * b] : 0.0, center2 ? center2[2 * b + 1] : 0.0, filter, b, b * (size_t)m_max};
    fe_gather_ranked(rows, s_key, s_wave, b, m_max, scores, score_type, keys, x1, x2, d1, d2, slot, n_out);
}

// k_gather_images with scores
template <typename KpT, typename DepthT>
__global__ __launch_bounds__(FE_THREADS) void k_gather_images_ranked(const KpT *__restrict__ kp, const int32_t *__restrict__ kp_count, int k_max,
                                                                     const DepthT *__restrict__ depth, const int32_t *__restrict__ size, int h_max,
                                                                     int w_max, const double *__restrict__ center, int n_images,
                                                                     const int32_t *__restrict__ pairs, const int32_t *__restrict__ matches, int m_max,
                                                                     int filter, const void *__restrict__ scores, int score_type, uint64_t *keys,
                                                                     double *__restrict__ x1, double *__restrict__ x2, double *__restrict__ d1,
                                                                     double *__restrict__ d2, int32_t *__restrict__ slot, int32_t *__restrict__ n_out) {
    __shared__ uint64_t s_key[RANK_TILE];
    __shared__ int s_wave[FE_THREADS / 64];
    const size_t b = blockIdx.x;
    const FeImageRows<KpT, DepthT> rows(kp, kp_count, k_max, depth, size, h_max, w_max, center, n_images, pairs, matches, filter, b, b * (size_t)m_max);
    fe_gather_ranked(rows, s_key, s_wave, b, m_max, scores, score_type, keys, x1, x2, d1, d2, slot, n_out);
}

// ---- the front end without depth maps: the four kernels above on FePointMatchRows / FePointImageRows.  One template parameter (the keypoint
// type), no depth buffer: d1 = d2 = nullptr into the shared compactions, which do not touch them (Rows::HAS_DEPTH).
template <typename KpT>
__global__ __launch_bounds__(FE_THREADS) void k_gather_points(const KpT *__restrict__ kp1, const KpT *__restrict__ kp2, int k1, int k2,
                                                              const int32_t *__restrict__ matches, int m_max, const double *__restrict__ center1,
                                                              const double *__restrict__ center2, double *__restrict__ x1, double *__restrict__ x2,
                                                              int32_t *__restrict__ slot, int32_t *__restrict__ n_out) {
    __shared__ int s_wave[FE_THREADS / 64];
    const size_t b = blockIdx.x;
    const FePointMatchRows<KpT> rows{kp1, kp2, k1, k2, matches, center1 ? center1[2 * b] : 0.0, center1 ? center1[2 * b + 1] : 0.0,
                                     center2 ? center2[2 * b] : 0.0, center2 ? center2[2 * b + 1] : 0.0, b, b * (size_t)m_max};
    fe_gather_ordered(rows, s_wave, b, m_max, x1, x2, nullptr, nullptr, slot, n_out);
}

template <typename KpT>
__global__ __launch_bounds__(FE_THREADS) void k_gather_points_images(const KpT *__restrict__ kp, const int32_t *__restrict__ kp_count, int k_max,
                                                                     const double *__restrict__ center, int n_images, const int32_t *__restrict__ pairs,
                                                                     const int32_t *__restrict__ matches, int m_max, double *__restrict__ x1,
                                                                     double *__restrict__ x2, int32_t *__restrict__ slot, int32_t *__restrict__ n_out) {
    __shared__ int s_wave[FE_THREADS / 64];
    const size_t b = blockIdx.x;
    const FePointImageRows<KpT> rows(kp, kp_count, k_max, center, n_images, pairs, matches, b, b * (size_t)m_max);
    fe_gather_ordered(rows, s_wave, b, m_max, x1, x2, nullptr, nullptr, slot, n_out);
}

template <typename KpT>
__global__ __launch_bounds__(FE_THREADS) void k_gather_points_ranked(const KpT *__restrict__ kp1, const KpT *__restrict__ kp2, int k1, int k2,
                                                                     const int32_t *__restrict__ matches, int m_max, const double *__restrict__ center1,
                                                                     const double *__restrict__ center2, const void *__restrict__ scores, int score_type,
                                                                     uint64_t *keys, double *__restrict__ x1, double *__restrict__ x2,
                                                                     int32_t *__restrict__ slot, int32_t *__restrict__ n_out) {
    __shared__ uint64_t s_key[RANK_TILE];
    __shared__ int s_wave[FE_THREADS / 64];
    const size_t b = blockIdx.x;
    const FePointMatchRows<KpT> rows{kp1, kp2, k1, k2, matches, center1 ? center1[2 * b] : 0.0, center1 ? center1[2 * b + 1] : 0.0,
                                     center2 ? center2[2 * b] : 0.0, center2 ? center2[2 * b + 1] : 0.0, b, b * (size_t)m_max};
    fe_gather_ranked(rows, s_key, s_wave, b, m_max, scores, score_type, keys, x1, x2, nullptr, nullptr, slot, n_out);
}

template <typename KpT>
__global__ __launch_bounds__(FE_THREADS) void k_gather_points_images_ranked(const KpT *__restrict__ kp, const int32_t *__restrict__ kp_count, int k_max,
                                                                            const double *__restrict__ center, int n_images,
                                                                            const int32_t *__restrict__ pairs, const int32_t *__restrict__ matches, int m_max,
                                                                            const void *__restrict__ scores, int score_type, uint64_t *keys,
                                                                            double *__restrict__ x1, double *__restrict__ x2, int32_t *__restrict__ slot,
                                                                            int32_t *__restrict__ n_out) {
    __shared__ uint64_t s_key[RANK_TILE];
    __shared__ int s_wave[FE_THREADS / 64];
    const size_t b = blockIdx.x;
    const FePointImageRows<KpT> rows(kp, kp_count, k_max, center, n_images, pairs, matches, b, b * (size_t)m_max);
    fe_gather_ranked(rows, s_key, s_wave, b, m_max, scores, score_type, keys, x1, x2, nullptr, nullptr, slot, n_out);
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
