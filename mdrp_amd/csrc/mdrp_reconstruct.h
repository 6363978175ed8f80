// mdrp_reconstruct.h — the back end (include/mdrp_reconstruct.h): from a batch of models and the pairs' depth maps to the fused two-view
// point cloud of every pair in camera 2's frame, subsampled, filtered and compacted on the device.
//
// mdrp_amd/frontend.py reconstruct_pair_numpy is the definition (rules R1-R7).  What decides whether a pixel is kept is an integer (the hash of its
// coordinates against a threshold) and a test of its depth; what is written for a kept pixel is a fixed sequence of float64 operations, one per
// arithmetic sign and none of them fused, rounded once to float32.  The device result equals the NumPy one as bytes.  The first part of this file is
// host + device arithmetic; the kernels follow behind __HIPCC__:
//   k_recon_count   a workgroup per tile of RECON_TILE consecutive pixels of one image of one pair, a lane per RECON_PER_LANE consecutive pixels: the
//                   tile's number of kept pixels (ballots and popcounts; a depth is read for a pixel the hash keeps, and for no other)
//   k_recon_scan    a workgroup per pair: each image's tile counts in place to their exclusive running sum, the pair's two true counts, and the
//                   pair's ReconPair: R, t, 1 / scale and the reciprocal focals, computed once per pair and side
//   k_recon_emit    the count kernel's walk again; a kept pixel's row is its image's start + its tile's offset + the kept pixels of the lower lanes
//                   (lane order is pixel order) + its place among its lane's own; it is unprojected, transformed (image 1), rounded and written
//                   while it fits.  The workgroups behind the tiles write the filler behind the last written row.
// Nothing is proportional to B * h * w but the tile counts (4 bytes per 1024 pixels).
//
// The pieces of the tile walk are shared with the scene kernels (mdrp_scene.h) and the co-visibility kernels (mdrp_covis.h): ReconWalk and recon_lane
// (R2-R4 for a lane), recon_side_lane (a pair's tile to its side, view and walk), recon_tile_total and recon_tile_rank (the compaction through one
// LDS word per wavefront), recon_fill (the filler) and recon_write_rows (the rows, around a functor for the point).  Two pieces stay where they were
// (profiles/backend_refactor_disasm.txt).  The "cameras of pair b, or null" selection in k_recon_scan and k_covis_pair: every shared form that was
// tried changed those kernels' registers.  The three-step scans of k_recon_scan (uint32, a barrier behind each side) and k_scene_scan (int64, one body
// whose every step branches on the phase): a shared helper would take k_scene_scan's phase 0 out of that body and so change its code.
#pragma once
#include <math.h>
#include <stdint.h>
#include "mdrp_dense.h" // dense_lowbias32 (D4's hash); through it mdrp_frontend.h: fe_isinf, fe_isfinite, fe_image_valid, fe_clamp_extent, FE_F32

namespace mdrp {

constexpr int RECON_KEEP_NOT_INF = 0, RECON_KEEP_FINITE = 1; // == MDRP_KEEP_NOT_INF, MDRP_KEEP_FINITE
constexpr int RECON_MAX_EXTENT = 65536;                      // == MDRP_RECON_MAX_EXTENT: v and u share the hash's 32-bit key
constexpr uint32_t RECON_ALL = 0xFFFFFFFFu;                  // == MDRP_RECON_ALL: the threshold that keeps every pixel
constexpr uint32_t RECON_STAGE_1 = 3, RECON_STAGE_2 = 4;     // D4's stages 1 and 2 are the dense sampler's
constexpr int RECON_MODEL_BYTES = 96;                        // sizeof(mdrp_model): the smallest stride of the model array

// R3.  The hash takes the seed, the image and the pixel, never the pair's position in the batch (v, u < 65536).
MDRP_HD uint32_t recon_hash(uint32_t seed, uint32_t stage, uint32_t v, uint32_t u) {
    return dense_lowbias32(seed * 0x9E3779B1u + stage * 0x85EBCA77u + ((v << 16) | u));
}
MDRP_HD bool recon_candidate(uint32_t thr, uint32_t seed, uint32_t stage, uint32_t v, uint32_t u) { return thr == RECON_ALL || recon_hash(seed, stage, v, u) < thr; }

// R4 on the widened depth
MDRP_HD bool recon_keep(double d, int keep) { return keep == RECON_KEEP_FINITE ? fe_isfinite(d) : !fe_isinf(d); }

// R1.  m: q[4] t[3] scale shift1 shift2 f1 f2 (mdrp_model)
MDRP_HD bool recon_usable(const double *m, int kind) {
    bool ok = true;
    for (int i = 0; i < 10; ++i) ok = ok && fe_isfinite(m[i]);
    ok = ok && m[7] != 0.0;
    if (kind != 0) ok = ok && fe_isfinite(m[10]) && fe_isfinite(m[11]) && m[10] > 0.0 && m[11] > 0.0;
    return ok;
}

// what a pixel needs of its pair: written once per pair by k_recon_scan.  A focal kind has ox = oy = 0 (x - 0.0 is x, bit for bit).
struct ReconSide {
    double rx, ry;   // 1.0 / fx, 1.0 / fy
    double ox, oy;   // the camera's principal point (calibrated kind)
    double shift;
};
struct ReconCam { int32_t model_id, pad_; double params[4]; }; // == mdrp_camera
struct ReconPair {
    ReconSide s[2];
    double R[9], t[3], inv; // image 1 alone: rotation from q, translation, 1.0 / scale
};

// A product that is rounded on its own.  The library is compiled with -ffp-contract=fast, under which the backend fuses a product into the sum that
// takes it whatever a pragma or a flag on the instruction says; the empty statement hides the product from it and emits no instruction.
MDRP_HD double recon_mul(double a, double b) {
    double r = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(r));
#endif
    return r;
}

// R5 alone: the point of pixel (v, u) with depth d in its own camera's frame; (c0, c1): its image's centre (shared with the scene kernels, mdrp_scene.h)
MDRP_HD void recon_unproject(const ReconSide &s, uint32_t v, uint32_t u, double c0, double c1, double d, double X[3]) {
    const double x = (double)u - c0, y = (double)v - c1;
    const double xn = (x - s.ox) * s.rx, yn = (y - s.oy) * s.ry;
    const double z = d + s.shift;
    X[0] = xn * z; X[1] = yn * z; X[2] = z;
}

// R5 and R6 for one kept pixel: every product and every sum is rounded on its own, as NumPy rounds them (a product that feeds a sum is a recon_mul).
// (v, u): the pixel; (c0, c1): its image's centre; d: its depth.  out: the point in camera 2's frame, before the rounding to float32.
MDRP_HD void recon_point(const ReconPair &p, int side, uint32_t v, uint32_t u, double c0, double c1, double d, double out[3]) {
    double X[3];
    recon_unproject(p.s[side], v, u, c0, c1, d, X);
    const double X0 = X[0], X1 = X[1], z = X[2];
    if (side != 0) {
        out[0] = X0; out[1] = X1; out[2] = z;
        return;
    }
    for (int r = 0; r < 3; ++r) {
        const double a = recon_mul(p.R[3 * r], X0), b = recon_mul(p.R[3 * r + 1], X1), c = recon_mul(p.R[3 * r + 2], z);
        out[r] = p.inv * (((a + b) + c) + p.t[r]);
    }
}

// one image's part of the record: from its camera (calibrated kind) or from the model's focal f
MDRP_HD ReconSide recon_side(int kind, int id, const double *c, double f, double shift) {
    ReconSide s;
    s.shift = shift;
    if (kind == 0) {
        const bool pinhole = id == 1;
        s.rx = 1.0 / c[0]; s.ry = 1.0 / (pinhole ? c[1] : c[0]);
        s.ox = pinhole ? c[2] : c[1]; s.oy = pinhole ? c[3] : c[2];
    } else {
        s.rx = s.ry = 1.0 / f;
        s.ox = s.oy = 0.0;
    }
    return s;
}

// R6's rotation from the model's q = (w, x, y, z), by the expressions of poselib._quat_to_R as they are written there (shared with mdrp_scene.h)
MDRP_HD void recon_rotation(const double *m, double R[9]) {
    const double w = m[0], x = m[1], y = m[2], z = m[3];
    const double xx = recon_mul(x, x), yy = recon_mul(y, y), zz = recon_mul(z, z), xy = recon_mul(x, y), xz = recon_mul(x, z), yz = recon_mul(y, z);
    const double wx = recon_mul(w, x), wy = recon_mul(w, y), wz = recon_mul(w, z);
    // (2 s is exact: 1 - 2 s rounds once, fused or not)
    R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz); R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz); R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy); R[7] = 2.0 * (yz + wx); R[8] = 1.0 - 2.0 * (xx + yy);
}
// the pair's record from its model and its two cameras (cam: model_id 0 {f, cx, cy}, 1 {fx, fy, cx, cy}; null for a focal kind)
MDRP_HD void recon_pair(const double *m, int kind, int id1, const double *cam1, int id2, const double *cam2, ReconPair &p) {
    recon_rotation(m, p.R);
    p.t[0] = m[4]; p.t[1] = m[5]; p.t[2] = m[6];
    p.inv = 1.0 / m[7];
    p.s[0] = recon_side(kind, id1, cam1, m[10], m[8]);
    p.s[1] = recon_side(kind, id2, cam2, m[11], m[9]);
}

#if defined(__HIPCC__)

constexpr int RECON_THREADS = 256;                            // four wavefronts
constexpr int RECON_PER_LANE = 4;                             // consecutive pixels of a lane
constexpr int RECON_TILE = RECON_THREADS * RECON_PER_LANE;    // pixels of a workgroup

// what the kernels take: both descriptors, flattened.  pairs == null is the per-pair form (maps [B][h][w], centres [B][2]); otherwise the per-image
// form: depth1 == depth2 and center1 == center2 are the image tables, h1 = h2 = h_max, w1 = w2 = w_max, size may be null.
struct ReconArgs {
    const void *depth1, *depth2;
    const double *center1, *center2;
    const int32_t *size, *pairs;
    const unsigned char *models; // [B] records model_stride bytes apart, an mdrp_model at the front of each
    const ReconCam *cam1, *cam2;   // [B], calibrated kind alone
    int model_stride, depth_type, kind, keep, n_images;
    int h1, w1, h2, w2;
    uint32_t thr, seed;
    int p_max;
    int nt1, nt2, nfill; // tiles of image 1 | of image 2 | filler workgroups, per pair
};

// one image of one pair: the map it reads, the valid region, the row stride
struct ReconView {
    size_t base;    // element offset of the map
    int h, w, stride;
    int image;      // row of the centre table
    bool ok;        // (per-image form) both indices of the pair address the set
};
__device__ __forceinline__ ReconView recon_view(const ReconArgs &a, size_t b, int side) {
    ReconView v;
    const int H = side ? a.h2 : a.h1, W = side ? a.w2 : a.w1;
    v.stride = W;
    if (!a.pairs) {
        v.ok = true; v.image = (int)b; v.h = H; v.w = W;
        v.base = b * (size_t)H * (size_t)W;
        return v;
    }
    const int i0 = a.pairs[2 * b], i1 = a.pairs[2 * b + 1];
    v.ok = fe_image_valid(i0, a.n_images) && fe_image_valid(i1, a.n_images);
    v.image = v.ok ? (side ? i1 : i0) : 0; // nothing is read through an index outside the set
    v.h = v.ok ? (a.size ? fe_clamp_extent(a.size[2 * (size_t)v.image], H) : H) : 0;
    v.w = v.ok ? (a.size ? fe_clamp_extent(a.size[2 * (size_t)v.image + 1], W) : W) : 0;
    v.base = (size_t)v.image * (size_t)H * (size_t)W;
    return v;
}

// what the lane walk reads of a call: the map, its element type, R4's filter and R3's threshold, seed and stage
struct ReconWalk {
    const void *map;
    int depth_type, keep;
    uint32_t thr, seed, stage;
};
// ... of one side (or direction) of a two-view call, whose stage is stage1 or stage2
__device__ __forceinline__ ReconWalk recon_walk(const ReconArgs &a, int side, uint32_t stage1, uint32_t stage2) {
    return {side ? a.depth2 : a.depth1, a.depth_type, a.keep, a.thr, a.seed, side ? stage2 : stage1};
}

// R2-R4 for the RECON_PER_LANE consecutive pixels of a lane that start at pixel p0 of a view with npix pixels: bit j of the result is set iff pixel
// p0 + j is kept; d[j], vv[j], uu[j] are its depth and coordinates.  One division per lane.
__device__ __forceinline__ unsigned recon_lane(const ReconWalk &k, const ReconView &vw, uint32_t npix, uint32_t p0, double d[RECON_PER_LANE],
                                               uint32_t vv[RECON_PER_LANE], uint32_t uu[RECON_PER_LANE]) {
    const void *map = k.map; // (both as locals: read through k inside the loop, the stage's product with the hash's constant is no longer folded)
    const uint32_t stage = k.stage;
    unsigned kept = 0;
    if (p0 >= npix) return 0; // (npix > 0: w > 0)
    uint32_t v = p0 / (uint32_t)vw.w, u = p0 - v * (uint32_t)vw.w;
#pragma unroll
    for (int j = 0; j < RECON_PER_LANE; ++j) {
        vv[j] = v; uu[j] = u; d[j] = 0.0;
        if (p0 + (uint32_t)j < npix && recon_candidate(k.thr, k.seed, stage, v, u)) {
            d[j] = dense_ld(map, k.depth_type, vw.base + (size_t)v * (size_t)vw.stride + (size_t)u);
            if (recon_keep(d[j], k.keep)) kept |= 1u << j;
        }
        if (++u == (uint32_t)vw.w) { u = 0; ++v; }
    }
    return kept;
}

// Tile `tile` of pair b, of the pair's nt1 tiles of image 1 and nt2 of image 2: its side, its view, whether the pair emits at all (R1; uniform over
// the workgroup), and this lane's walk of it under the side's stage.
struct ReconSideTile {
    int side;
    ReconView vw;
    bool usable;
};
__device__ __forceinline__ unsigned recon_side_lane(const ReconArgs &a, size_t b, int tile, int tid, uint32_t stage1, uint32_t stage2, ReconSideTile &t,
                                                    double d[RECON_PER_LANE], uint32_t vv[RECON_PER_LANE], uint32_t uu[RECON_PER_LANE]) {
    t.side = tile >= a.nt1 ? 1 : 0;
    const int ts = t.side ? tile - a.nt1 : tile;
    t.vw = recon_view(a, b, t.side);
    t.usable = t.vw.ok && recon_usable(reinterpret_cast<const double *>(a.models + b * (size_t)a.model_stride), a.kind);
    const uint32_t npix = t.usable ? (uint32_t)t.vw.h * (uint32_t)t.vw.w : 0u;
    return recon_lane(recon_walk(a, t.side, stage1, stage2), t.vw, npix, (uint32_t)ts * RECON_TILE + (uint32_t)tid * RECON_PER_LANE, d, vv, uu);
}

// The kept pixels of a tile from its lanes' masks, through s_wave (one word per wavefront): the count kernels' tail.  Thread 0 writes the sum to *out.
__device__ __forceinline__ void recon_tile_total(unsigned kept, int tid, uint32_t *s_wave /*LDS, RECON_THREADS / 64*/, uint32_t *out) {
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < RECON_PER_LANE; ++j) c += (uint32_t)__popcll(__ballot((kept >> j) & 1u));
    if (lane == 0) s_wave[wave] = c;
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < RECON_THREADS / 64; ++w) total += s_wave[w];
        *out = total;
    }
}

// The kept pixels of the tile before this lane's own, through s_wave: lanes take consecutive runs of pixels, so lane order is pixel order.
__device__ __forceinline__ uint32_t recon_tile_rank(unsigned kept, int tid, uint32_t *s_wave /*LDS, RECON_THREADS / 64*/) {
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t before = 0, c = 0;
#pragma unroll
    for (int j = 0; j < RECON_PER_LANE; ++j) {
        const unsigned long long ball = __ballot((kept >> j) & 1u);
        before += (uint32_t)__popcll(ball & below);
        c += (uint32_t)__popcll(ball);
    }
    if (lane == 0) s_wave[wave] = c;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < RECON_THREADS / 64; ++w) before += w < wave ? s_wave[w] : 0u;
    return before;
}

// A filler workgroup: the RECON_TILE rows from `first` on that lie behind the last written row and inside the cloud
__device__ __forceinline__ void recon_fill(int64_t first, int tid, int64_t written, int64_t p_max, float *pts, int32_t *pix) {
#pragma unroll
    for (int j = 0; j < RECON_PER_LANE; ++j) {
        const int64_t r = first + (int64_t)j * RECON_THREADS + tid;
        if (r >= written && r < p_max) {
            pts[3 * r] = 0.0f; pts[3 * r + 1] = 0.0f; pts[3 * r + 2] = 0.0f;
            pix[r] = -1;
        }
    }
}

// A lane's kept pixels to the rows from `row` on, written while they fit (the counts stay the true ones).  point(v, u, d, out[3]): R5 and R6 (or the
// scene's S5 and S6) of one pixel, rounded here to float32; stride: the row stride of the pixel's map.
template <typename Point>
__device__ __forceinline__ void recon_write_rows(unsigned kept, int64_t row, int64_t p_max, const uint32_t vv[RECON_PER_LANE], const uint32_t uu[RECON_PER_LANE],
                                                 const double d[RECON_PER_LANE], int stride, Point point, float *pts, int32_t *pix) {
#pragma unroll
    for (int j = 0; j < RECON_PER_LANE; ++j) {
        if (!((kept >> j) & 1u)) continue;
        if (row < p_max) {
            double o[3];
            point(vv[j], uu[j], d[j], o);
            pts[3 * row] = (float)o[0]; pts[3 * row + 1] = (float)o[1]; pts[3 * row + 2] = (float)o[2];
            pix[row] = (int32_t)(vv[j] * (uint32_t)stride + uu[j]);
        }
        ++row;
    }
}

MDRP_GLOBAL __launch_bounds__(RECON_THREADS) void k_recon_count(ReconArgs a, uint32_t *__restrict__ tcnt) {
    __shared__ uint32_t s_wave[RECON_THREADS / 64];
    const int nt = a.nt1 + a.nt2;
    const size_t b = blockIdx.x / (uint32_t)nt;
    const int tile = (int)(blockIdx.x % (uint32_t)nt), tid = threadIdx.x;
    ReconSideTile t;
    double d[RECON_PER_LANE];
    uint32_t vv[RECON_PER_LANE], uu[RECON_PER_LANE];
    recon_tile_total(recon_side_lane(a, b, tile, tid, RECON_STAGE_1, RECON_STAGE_2, t, d, vv, uu), tid, s_wave, tcnt + (b * (size_t)nt + tile));
}

// One workgroup per pair.  Each image's tile counts to their exclusive running sum in place, as k_dense_scan sums its blocks: a thread sums its run
// of consecutive tiles, thread 0 scans the run totals, the thread walks its run again.  (tcnt is read and written by the same thread only.)  Thread 0
// writes the pair's true counts and its ReconPair.
MDRP_GLOBAL __launch_bounds__(RECON_THREADS) void k_recon_scan(ReconArgs a, uint32_t *tcnt, ReconPair *__restrict__ rp, int32_t *__restrict__ counts) {
    __shared__ uint32_t s_run[RECON_THREADS];
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x;
    uint32_t *cnt = tcnt + b * (size_t)(a.nt1 + a.nt2);
    for (int side = 0; side < 2; ++side) {
        const int nt = side ? a.nt2 : a.nt1;
        const int per = (nt + RECON_THREADS - 1) / RECON_THREADS, lo = min(tid * per, nt), hi = min(lo + per, nt);
        uint32_t sum = 0;
        for (int i = lo; i < hi; ++i) sum += cnt[i];
        s_run[tid] = sum;
        __syncthreads();
        if (tid == 0) {
            uint32_t run = 0;
            for (int t = 0; t < RECON_THREADS; ++t) {
                const uint32_t v = s_run[t];
                s_run[t] = run; // exclusive
                run += v;
            }
            counts[2 * b + side] = (int32_t)run; // (a map has fewer than 2^31 pixels)
        }
        __syncthreads();
        uint32_t run = s_run[tid];
        for (int i = lo; i < hi; ++i) { const uint32_t v = cnt[i]; cnt[i] = run; run += v; }
        __syncthreads(); // s_run is rewritten for image 2
        cnt += nt;
    }
    if (tid == 0) {
        const ReconCam *c1 = a.kind == 0 ? a.cam1 + b : nullptr, *c2 = a.kind == 0 ? a.cam2 + b : nullptr;
        ReconPair p;
        recon_pair(reinterpret_cast<const double *>(a.models + b * (size_t)a.model_stride), a.kind, c1 ? c1->model_id : 0, c1 ? c1->params : nullptr,
                   c2 ? c2->model_id : 0, c2 ? c2->params : nullptr, p);
        rp[b] = p;
    }
}

// Grid: per pair nt1 + nt2 tiles, then nfill filler workgroups.  (counts and tcnt are k_recon_scan's.)
MDRP_GLOBAL __launch_bounds__(RECON_THREADS) void k_recon_emit(ReconArgs a, const uint32_t *__restrict__ tcnt, const ReconPair *__restrict__ rp,
                                                              const int32_t *__restrict__ counts, float *__restrict__ points, int32_t *__restrict__ pixel) {
    const int nt = a.nt1 + a.nt2, per_pair = nt + a.nfill;
    const size_t b = blockIdx.x / (uint32_t)per_pair;
    const int tile = (int)(blockIdx.x % (uint32_t)per_pair), tid = threadIdx.x;
    const int64_t n1 = counts[2 * b], n2 = counts[2 * b + 1], p_max = a.p_max;
    const int64_t start2 = n1 < p_max ? n1 : p_max; // image 2's first row
    float *pts = points + b * (size_t)a.p_max * 3;
    int32_t *pix = pixel + b * (size_t)a.p_max;
    if (tile >= nt) { // the filler behind the last written row
        recon_fill((int64_t)(tile - nt) * RECON_TILE, tid, start2 + (n2 < p_max - start2 ? n2 : p_max - start2), p_max, pts, pix);
        return;
    }
    __shared__ uint32_t s_wave[RECON_THREADS / 64];
    ReconSideTile t;
    double d[RECON_PER_LANE];
    uint32_t vv[RECON_PER_LANE], uu[RECON_PER_LANE];
    const unsigned kept = recon_side_lane(a, b, tile, tid, RECON_STAGE_1, RECON_STAGE_2, t, d, vv, uu);
    const uint32_t before = recon_tile_rank(kept, tid, s_wave);
    if (!kept) return;
    const int side = t.side;
    const int64_t row = (side ? start2 : 0) + (int64_t)tcnt[b * (size_t)nt + tile] + (int64_t)before;
    const ReconPair &p = rp[b];
    const double *ctr = side ? a.center2 : a.center1;
    const double c0 = ctr ? ctr[2 * (size_t)t.vw.image] : 0.0, c1 = ctr ? ctr[2 * (size_t)t.vw.image + 1] : 0.0;
    const auto point = [&p, side, c0, c1](uint32_t v, uint32_t u, double dd, double o[3]) { recon_point(p, side, v, u, c0, c1, dd, o); };
    recon_write_rows(kept, row, p_max, vv, uu, d, t.vw.stride, point, pts, pix);
}

#endif // __HIPCC__

} // namespace mdrp
