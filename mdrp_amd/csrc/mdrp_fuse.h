// mdrp_fuse.h — the consistency filter of a scene (include/mdrp_fuse.h): the scene's cloud (mdrp_scene.h) with a decision in front of the
// compaction.  A candidate pixel's point in its root's frame is carried into the camera frame of each of its image's views, projected to the nearest
// pixel of that view's depth map and compared with the depth there (rules C5 and C6 of mdrp_covis.h); the point is kept iff enough views are
// consistent with it and few enough see through it.
//
// mdrp_amd/frontend.py fuse_scene_numpy is the definition (rules F1-F6).  Every count is an integer; every quantity that decides one is a fixed
// sequence of float64 operations, one rounding per arithmetic sign, none of them fused, IEEE division.  The device result equals the NumPy one as
// bytes.  The first part of this file is host + device arithmetic - fuse_decide is the ONE function through which both passes and the host build
// (tests/hostmath/fuse_host.cpp) decide; the kernels follow behind __HIPCC__:
//   k_fuse_views   a lane per image: its FuseView (what a point needs of the image as a VIEW: the record to invert, the camera to project with, the
//                  centre, the valid region, the map's offset) and its FuseRow (F3: the valid slots of its row of `views`, compacted)
//   k_fuse_count   k_scene_count's walk; a workgroup's tile belongs to one image, so its FuseRow and the FuseViews it names are read from uniform
//                  addresses, once per slot for the lane's RECON_PER_LANE pixels; only the target-depth gather diverges.  The tile's KEPT count.
//   k_fuse_emit    the same walk and the same decision again (nothing per pixel is left between the passes), ranked by recon_tile_rank; rows and
//                  support written while they fit.  The workgroups behind the tiles write the filler.
// k_scene_chain (the records), k_scene_scan (the running sums) and recon_fill (the filler of points and pixel) are used as they are.  The scratch is
// per image (184 + 36 bytes) and per tile (4 bytes); nothing is proportional to h * w * V.
#pragma once
#include "mdrp_covis.h"
#include "mdrp_scene.h"

namespace mdrp {

constexpr int FUSE_MAX_VIEWS = 8; // == MDRP_FUSE_MAX_VIEWS

// what a point needs of an image it is tested against: written once per image by k_fuse_views
struct FuseView {
    double R[9], t[3], s;  // the image's record: F4 inverts it
    double fx, fy, ox, oy; // C5's camera: the image's own (calibrated kind), or its record's focal with ox = oy = 0
    double shift, c0, c1;  // its shift and its centre
    size_t base;           // element offset of its map
    int32_t h, w;          // its valid region
    int32_t root, depth;   // of its record (depth 0: the point is in its frame already)
};
// F3 for one image: the n valid slots of its row of `views`, in the row's order
struct FuseRow { int32_t n, view[FUSE_MAX_VIEWS]; };
// C6's band and F6's gate
struct FuseGate { double lo, hi; int32_t min_consistent, max_violating; };

MDRP_HD FuseView fuse_view(const SceneTransform &T, int kind, const ReconCam *cam, double c0, double c1, int h, int w, size_t base) {
    FuseView g;
#pragma unroll
    for (int k = 0; k < 9; ++k) g.R[k] = T.R[k];
    g.t[0] = T.t[0]; g.t[1] = T.t[1]; g.t[2] = T.t[2];
    g.s = T.s; g.shift = T.shift; g.c0 = c0; g.c1 = c1;
    g.base = base; g.h = h; g.w = w; g.root = T.root; g.depth = T.depth;
    g.fx = g.fy = g.ox = g.oy = 0.0;
    if (T.depth < 0) return g; // (never a valid slot)
    const ReconSide s = recon_side(kind, cam ? cam->model_id : 0, cam ? cam->params : nullptr, T.f, T.shift);
    g.ox = s.ox; g.oy = s.oy;
    covis_focals(kind, cam ? cam->model_id : 0, cam ? cam->params : nullptr, T.f, g.fx, g.fy);
    return g;
}

// F3: row[0 .. n_views) of image i -> its valid slots.  Nothing is read through an inert slot.
MDRP_HD void fuse_slots(const SceneTransform *T, int n_images, int i, const int32_t *row, int n_views, FuseRow &r) {
    r.n = 0;
#pragma unroll
    for (int k = 0; k < FUSE_MAX_VIEWS; ++k) r.view[k] = -1;
    if (T[i].depth < 0) return;
#pragma unroll
    for (int k = 0; k < FUSE_MAX_VIEWS; ++k) { // (every index of r.view is a constant: the row stays in registers)
        if (k >= n_views) continue;
        const int n = row[k];
        if (!fe_image_valid(n, n_images) || n == i) continue;
        if (T[n].depth < 0 || T[n].root != T[i].root) continue;
        bool seen = false;
#pragma unroll
        for (int e = 0; e < k; ++e) seen = seen || r.view[e] == n;
        if (seen) continue;
#pragma unroll
        for (int e = 0; e <= k; ++e)
            if (e == r.n) r.view[e] = n;
        ++r.n;
    }
}

// F4 and F5 for one point Q of the root's frame and one view: C7's class bits FRONT, INSIDE, KNOWN and one of CONSISTENT, OCCLUDED, VIOLATING.
// ld(g, vt, ut): the view's depth at a pixel inside its valid region, widened to double; called for an INSIDE point and for no other.
// (The projection is covis_project's lines on a view's own fields: that function reads a pair's record, and the co-visibility kernels' code is pinned.)
template <typename Load>
MDRP_HD unsigned fuse_slot(const FuseView &g, const double Q[3], double lo, double hi, Load ld) {
    double P[3];
    if (g.depth == 0) {
        P[0] = Q[0]; P[1] = Q[1]; P[2] = Q[2];
    } else {
        double Y[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) Y[r] = recon_mul(g.s, Q[r]) - g.t[r];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double a = recon_mul(g.R[r], Y[0]), b = recon_mul(g.R[3 + r], Y[1]), c = recon_mul(g.R[6 + r], Y[2]);
            P[r] = (a + b) + c;
        }
    }
    if (!(fe_isfinite(P[2]) && P[2] > 0.0)) return 0;
    const double xo = P[0] / P[2], yo = P[1] / P[2];
    const double px = (recon_mul(xo, g.fx) + g.ox) + g.c0, py = (recon_mul(yo, g.fy) + g.oy) + g.c1;
    const double a = px + 0.5, b = py + 0.5; // the nearest pixel
    if (!(a >= 0.0 && a < (double)g.w && b >= 0.0 && b < (double)g.h)) return 1u << COVIS_FRONT; // (a NaN fails)
    const uint32_t ut = (uint32_t)(int)a, vt = (uint32_t)(int)b;
    return (1u << COVIS_FRONT) | (1u << COVIS_INSIDE) | covis_compare(P[2], ld(g, vt, ut), g.shift, lo, hi);
}

// F2-F6 for N candidates of one image: bit j of cand: pixel j is a candidate (S3, S4); d[j]: its depth; Q[j]: its point (F1), read where the image has
// a valid slot.  support[j] = n_cons | n_viol << 8; the result's bit j: the gate keeps pixel j.  The views are walked in the outer loop: one view's
// fields serve the N pixels, whose N gathers are in flight together.
template <int N, typename Load>
MDRP_HD unsigned fuse_decide(unsigned cand, const double d[N], double shift, const double Q[N][3], const FuseRow &row, const FuseView *views,
                             const FuseGate &gate, Load ld, unsigned support[N]) {
    unsigned tested = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        support[j] = 0;
        if (((cand >> j) & 1u) && covis_depth_ok(d[j], shift)) tested |= 1u << j; // F2
    }
    for (int k = 0; k < row.n; ++k) {
        const FuseView &g = views[row.view[k]];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if (!((tested >> j) & 1u)) continue;
            const unsigned c = fuse_slot(g, Q[j], gate.lo, gate.hi, ld);
            support[j] += ((c >> COVIS_CONSISTENT) & 1u) + (((c >> COVIS_VIOLATING) & 1u) << 8);
        }
    }
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (((cand >> j) & 1u) && (int)(support[j] & 0xFFu) >= gate.min_consistent && (int)(support[j] >> 8) <= gate.max_violating) keep |= 1u << j; // F6
    return keep;
}

#if defined(__HIPCC__)

// what the pixel kernels take beside the scene's: the tables of k_fuse_views and the gate
struct FuseArgs {
    const FuseView *views; // [n_images]
    const FuseRow *rows;   // [n_images]
    FuseGate gate;
};

// Grid: ceil(n_images / SCENE_CHAIN_THREADS).  T: k_scene_chain's records; views: [n_images][n_views] or null (n_views == 0).
MDRP_GLOBAL __launch_bounds__(SCENE_CHAIN_THREADS) void k_fuse_views(SceneArgs a, int kind, const ReconCam *__restrict__ cams, const SceneTransform *__restrict__ T,
                                                                    const int32_t *__restrict__ views, int n_views, FuseView *__restrict__ fv,
                                                                    FuseRow *__restrict__ fr) {
    const int i = (int)(blockIdx.x * SCENE_CHAIN_THREADS + threadIdx.x);
    if (i >= a.n_images) return;
    const bool attached = T[i].depth >= 0;
    const ReconView vw = scene_view(a, (size_t)i, attached);
    const double c0 = a.center ? a.center[2 * (size_t)i] : 0.0, c1 = a.center ? a.center[2 * (size_t)i + 1] : 0.0;
    fv[i] = fuse_view(T[i], kind, cams ? cams + i : nullptr, c0, c1, vw.h, vw.w, vw.base);
    FuseRow r;
    fuse_slots(T, a.n_images, i, views + (size_t)i * (size_t)n_views, n_views, r);
    fr[i] = r;
}

// This lane's candidates of tile `tile` of an image (scene_lane), their points where they are needed, and the decision: the kept pixels' mask.
// points: Q is computed whether or not a slot asks for it (the emit pass writes it).
__device__ __forceinline__ unsigned fuse_lane(const SceneArgs &a, const FuseArgs &f, const SceneTransform *__restrict__ T, const SceneImage *__restrict__ im,
                                              size_t image, int tile, int tid, bool points, ReconView &vw, uint32_t vv[RECON_PER_LANE],
                                              uint32_t uu[RECON_PER_LANE], double Q[RECON_PER_LANE][3], unsigned support[RECON_PER_LANE]) {
    const SceneTransform &t = T[image];
    double d[RECON_PER_LANE];
    const unsigned cand = scene_lane(a, image, tile, tid, t.depth >= 0, vw, d, vv, uu);
    const FuseRow &row = f.rows[image];
    if (points || row.n > 0) { // (uniform over the workgroup)
        const SceneImage &si = im[image];
        const double c0 = a.center ? a.center[2 * image] : 0.0, c1 = a.center ? a.center[2 * image + 1] : 0.0;
#pragma unroll
        for (int j = 0; j < RECON_PER_LANE; ++j)
            if ((cand >> j) & 1u) scene_point(t, si, vv[j], uu[j], c0, c1, d[j], Q[j]);
    }
    const void *map = a.depth;
    const int type = a.depth_type;
    const size_t stride = (size_t)a.w;
    // (vt < g.h, ut < g.w: inside the view's valid region, which lies inside its allocation; g.base: the map of an image of the set)
    const auto ld = [map, type, stride](const FuseView &g, uint32_t vt, uint32_t ut) { return dense_ld(map, type, g.base + (size_t)vt * stride + (size_t)ut); };
    return fuse_decide<RECON_PER_LANE>(cand, d, t.shift, Q, row, f.views, f.gate, ld, support);
}

// Grid: n_images * nt tiles.
MDRP_GLOBAL __launch_bounds__(RECON_THREADS) void k_fuse_count(SceneArgs a, FuseArgs f, const SceneTransform *__restrict__ T, const SceneImage *__restrict__ im,
                                                              uint32_t *__restrict__ tcnt) {
    __shared__ uint32_t s_wave[RECON_THREADS / 64];
    const size_t image = blockIdx.x / (uint32_t)a.nt;
    const int tile = (int)(blockIdx.x % (uint32_t)a.nt), tid = threadIdx.x;
    ReconView vw;
    uint32_t vv[RECON_PER_LANE], uu[RECON_PER_LANE];
    double Q[RECON_PER_LANE][3];
    unsigned support[RECON_PER_LANE];
    recon_tile_total(fuse_lane(a, f, T, im, image, tile, tid, false, vw, vv, uu, Q, support), tid, s_wave, tcnt + blockIdx.x);
}

// Grid: n_images * nt tiles, then the filler workgroups.  (tcnt and offsets are k_scene_scan's.)
MDRP_GLOBAL __launch_bounds__(RECON_THREADS) void k_fuse_emit(SceneArgs a, FuseArgs f, const uint32_t *__restrict__ tcnt, const SceneTransform *__restrict__ T,
                                                             const SceneImage *__restrict__ im, const int64_t *__restrict__ offsets,
                                                             float *__restrict__ points, int32_t *__restrict__ pixel, uint8_t *__restrict__ sup) {
    const uint32_t tiles = (uint32_t)a.n_images * (uint32_t)a.nt; // (fits: the entry point checks the grid)
    const int tid = threadIdx.x;
    const int64_t p_max = a.p_max;
    if (blockIdx.x >= tiles) { // the filler behind the last written row
        const int64_t all = offsets[a.n_images], written = all < p_max ? all : p_max, first = (int64_t)(blockIdx.x - tiles) * RECON_TILE;
        recon_fill(first, tid, written, p_max, points, pixel);
#pragma unroll
        for (int j = 0; j < RECON_PER_LANE; ++j) {
            const int64_t r = first + (int64_t)j * RECON_THREADS + tid;
            if (r >= written && r < p_max) { sup[2 * r] = 0; sup[2 * r + 1] = 0; }
        }
        return;
    }
    __shared__ uint32_t s_wave[RECON_THREADS / 64];
    const size_t image = blockIdx.x / (uint32_t)a.nt;
    const int tile = (int)(blockIdx.x % (uint32_t)a.nt);
    ReconView vw;
    uint32_t vv[RECON_PER_LANE], uu[RECON_PER_LANE];
    double Q[RECON_PER_LANE][3];
    unsigned support[RECON_PER_LANE];
    const unsigned kept = fuse_lane(a, f, T, im, image, tile, tid, true, vw, vv, uu, Q, support);
    const uint32_t before = recon_tile_rank(kept, tid, s_wave);
    if (!kept) return;
    int64_t row = offsets[image] + (int64_t)tcnt[blockIdx.x] + (int64_t)before;
#pragma unroll
    for (int j = 0; j < RECON_PER_LANE; ++j) { // (recon_write_rows with the point at hand and the support beside it)
        if (!((kept >> j) & 1u)) continue;
        if (row < p_max) {
            points[3 * row] = (float)Q[j][0]; points[3 * row + 1] = (float)Q[j][1]; points[3 * row + 2] = (float)Q[j][2];
            pixel[row] = (int32_t)(vv[j] * (uint32_t)vw.stride + uu[j]);
            sup[2 * row] = (uint8_t)(support[j] & 0xFFu); sup[2 * row + 1] = (uint8_t)(support[j] >> 8);
        }
        ++row;
    }
}

#endif // __HIPCC__

} // namespace mdrp
