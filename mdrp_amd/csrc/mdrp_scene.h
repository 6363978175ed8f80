// mdrp_scene.h — the back end for an image set (include/mdrp_scene.h): the pairs' models chained along a tree into one transform per
// image, and the fused point cloud of the whole set, every image unprojected once into its root's frame.
//
// mdrp_amd/frontend.py scene_transforms_numpy / reconstruct_scene_numpy are the definition (rules S1-S6).  The tree walk has a fixed order and every
// product that feeds a sum is a recon_mul, so the transform records are defined as bytes; the subsample, the filter and the unprojection are
// mdrp_reconstruct.h's own device functions (recon_lane, recon_unproject) on a stage and a seed of the scene's.  The first part of this file is host +
// device arithmetic; the kernels follow behind __HIPCC__:
//   k_scene_chain   a lane per image: S1 and S2, the image's mdrp_scene_transform and its SceneImage (what a pixel needs of its image)
//   k_scene_count   a workgroup per tile of RECON_TILE consecutive pixels of one IMAGE, a lane per RECON_PER_LANE pixels: the tile's kept pixels
//   k_scene_scan    launched twice.  phase 0, a workgroup per image: its tile counts in place to their exclusive running sum, its true count to
//                   offsets[image + 1].  phase 1, one workgroup: the counts in place to the running sum over the images (int64)
//   k_scene_emit    the count kernel's walk again; row = offsets[image] + the tile's offset + the kept pixels of the lower lanes + the place among
//                   the lane's own; unprojected, carried to the root's frame, rounded, written while it fits.  The workgroups behind the tiles
//                   write the filler behind the last written row.
#pragma once
#include "mdrp_reconstruct.h"

namespace mdrp {

constexpr int SCENE_ABSENT = 0, SCENE_EDGE = 1, SCENE_ROOT = 2; // == MDRP_SCENE_*
constexpr uint32_t SCENE_STAGE = 5;                             // R3's stage of a scene (3 and 4 are the two-view back end's)
constexpr uint32_t SCENE_SEED_MUL = 0xC2B2AE35u;

struct SceneTransform { double R[9], t[3], s, f, shift; int32_t root, depth; }; // == mdrp_scene_transform
struct SceneImage { ReconSide side; double inv; };                               // the image's intrinsics and shift (R5) and 1.0 / s of its record

// S3: the image in the seed's place
MDRP_HD uint32_t scene_seed(uint32_t seed, uint32_t image) { return dense_lowbias32(seed + SCENE_SEED_MUL * (image + 1u)); }

// the scene as the chain reads it
struct SceneTree {
    const unsigned char *models; // [batch] records model_stride bytes apart
    const int32_t *pairs, *tree; // [batch][2] | [n_images][2]
    int model_stride, kind, batch, n_images;
};

struct SceneEdge { double R[9], t[3], s, f, shift; int other; };

// S1 for image i (in [0, n_images)): 0 where it is absent or detached by its own entry, else its role, with e its edge - a point X of image i is
// (e.R X + e.t) / e.s in the other image's frame - and its own focal and shift.  Nothing is read through a bad index.
MDRP_HD int scene_edge(const SceneTree &s, int i, SceneEdge &e) {
    const int p = s.tree[2 * (size_t)i], role = s.tree[2 * (size_t)i + 1];
#pragma unroll
    for (int k = 0; k < 9; ++k) e.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    e.t[0] = e.t[1] = e.t[2] = 0.0;
    e.s = 1.0; e.f = 0.0; e.shift = 0.0; e.other = -1;
    if (role != SCENE_EDGE && role != SCENE_ROOT) return 0;
    if (role == SCENE_ROOT && p == -1) return s.kind == 0 ? SCENE_ROOT : 0;
    if (p < 0 || p >= s.batch) return 0;
    const int a = s.pairs[2 * (size_t)p], c = s.pairs[2 * (size_t)p + 1];
    if (a == c || (i != a && i != c)) return 0;
    const int other = i == a ? c : a;
    if (!fe_image_valid(other, s.n_images)) return 0;
    const double *m = reinterpret_cast<const double *>(s.models + (size_t)p * (size_t)s.model_stride);
    if (!recon_usable(m, s.kind)) return 0;
    const bool first = i == a;
    e.other = other;
    e.shift = first ? m[8] : m[9];
    e.f = s.kind == 0 ? 0.0 : (first ? m[10] : m[11]);
    if (role == SCENE_ROOT) return SCENE_ROOT;
    double R[9];
    recon_rotation(m, R);
    if (first) { // the model itself
#pragma unroll
        for (int k = 0; k < 9; ++k) e.R[k] = R[k];
        e.t[0] = m[4]; e.t[1] = m[5]; e.t[2] = m[6];
        e.s = m[7];
    } else {     // its inverse
        const double inv = 1.0 / m[7];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c2 = 0; c2 < 3; ++c2) e.R[3 * r + c2] = R[3 * c2 + r];
            const double u = (recon_mul(R[r], m[4]) + recon_mul(R[3 + r], m[5])) + recon_mul(R[6 + r], m[6]);
            e.t[r] = -(u * inv);
        }
        e.s = inv;
    }
    return SCENE_EDGE;
}

// S2 for image i: its record
MDRP_HD void scene_chain(const SceneTree &s, int i, SceneTransform &T) {
#pragma unroll
    for (int k = 0; k < 9; ++k) T.R[k] = 0.0;
    T.t[0] = T.t[1] = T.t[2] = 0.0;
    T.s = T.f = T.shift = 0.0;
    T.root = T.depth = -1;
    SceneEdge e;
    const int role = scene_edge(s, i, e);
    if (!role) return;
    int root = -1, depth = 0;
    if (role == SCENE_ROOT) {
        root = i;
    } else {
        depth = 1;
        int node = e.other;
        for (int step = 0; step < s.n_images; ++step) { // cut after I steps: a cycle ends as detached
            SceneEdge n;
            const int rn = scene_edge(s, node, n);
            if (!rn) break;
            if (rn == SCENE_ROOT) { root = node; break; }
            double Rn[9], tn[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    Rn[3 * r + c] = (recon_mul(n.R[3 * r], e.R[c]) + recon_mul(n.R[3 * r + 1], e.R[3 + c])) + recon_mul(n.R[3 * r + 2], e.R[6 + c]);
                tn[r] = ((recon_mul(n.R[3 * r], e.t[0]) + recon_mul(n.R[3 * r + 1], e.t[1])) + recon_mul(n.R[3 * r + 2], e.t[2])) + recon_mul(e.s, n.t[r]);
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) e.R[k] = Rn[k];
            e.t[0] = tn[0]; e.t[1] = tn[1]; e.t[2] = tn[2];
            e.s = e.s * n.s;
            ++depth;
            node = n.other;
        }
        if (root < 0) return;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) T.R[k] = e.R[k];
    T.t[0] = e.t[0]; T.t[1] = e.t[1]; T.t[2] = e.t[2];
    T.s = e.s; T.f = e.f; T.shift = e.shift;
    T.root = root; T.depth = depth;
}

// what a pixel needs of its image, from the image's record and its camera (calibrated kind; null for a focal kind).  A detached image: zeros.
MDRP_HD SceneImage scene_image(const SceneTransform &T, int kind, const ReconCam *cam) {
    SceneImage im;
    if (T.depth < 0) {
        im.side.rx = im.side.ry = im.side.ox = im.side.oy = im.side.shift = 0.0;
        im.inv = 0.0;
        return im;
    }
    im.side = recon_side(kind, cam ? cam->model_id : 0, cam ? cam->params : nullptr, T.f, T.shift);
    im.inv = 1.0 / T.s;
    return im;
}

// S5 and S6 for one kept pixel of an image: the point in its root's frame, before the rounding to float32
MDRP_HD void scene_point(const SceneTransform &T, const SceneImage &im, uint32_t v, uint32_t u, double c0, double c1, double d, double out[3]) {
    double X[3];
    recon_unproject(im.side, v, u, c0, c1, d, X);
    if (T.depth == 0) { // a root's points are X as it stands
        out[0] = X[0]; out[1] = X[1]; out[2] = X[2];
        return;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double a = recon_mul(T.R[3 * r], X[0]), b = recon_mul(T.R[3 * r + 1], X[1]), c = recon_mul(T.R[3 * r + 2], X[2]);
        out[r] = (((a + b) + c) + T.t[r]) * im.inv;
    }
}

#if defined(__HIPCC__)

constexpr int SCENE_CHAIN_THREADS = 64;

// what the scene's pixel kernels take: mdrp_depth_image_pairs and mdrp_reconstruct_opt, flattened
struct SceneArgs {
    const void *depth;       // [n_images][h][w]
    const double *center;    // [n_images][2] or null
    const int32_t *size;     // [n_images][2] or null
    int depth_type, keep, n_images, h, w;
    uint32_t thr, seed;
    int p_max;
    int nt;                  // tiles per image
};

MDRP_GLOBAL __launch_bounds__(SCENE_CHAIN_THREADS) void k_scene_chain(SceneTree s, const ReconCam *__restrict__ cams, SceneTransform *__restrict__ T,
                                                                     SceneImage *__restrict__ im) {
    const int i = (int)(blockIdx.x * SCENE_CHAIN_THREADS + threadIdx.x);
    if (i >= s.n_images) return;
    SceneTransform t;
    scene_chain(s, i, t);
    T[i] = t;
    if (im) im[i] = scene_image(t, s.kind, cams ? cams + i : nullptr);
}

// the view of one image of the set (an image that emits nothing has no pixels)
__device__ __forceinline__ ReconView scene_view(const SceneArgs &a, size_t image, bool attached) {
    ReconView v;
    v.ok = attached; v.image = (int)image; v.stride = a.w;
    v.h = attached ? (a.size ? fe_clamp_extent(a.size[2 * image], a.h) : a.h) : 0;
    v.w = attached ? (a.size ? fe_clamp_extent(a.size[2 * image + 1], a.w) : a.w) : 0;
    v.base = image * (size_t)a.h * (size_t)a.w;
    return v;
}
// this lane's walk of tile `tile` of an image under S3's seed and the scene's stage; vw: the image's view
__device__ __forceinline__ unsigned scene_lane(const SceneArgs &a, size_t image, int tile, int tid, bool attached, ReconView &vw, double d[RECON_PER_LANE],
                                               uint32_t vv[RECON_PER_LANE], uint32_t uu[RECON_PER_LANE]) {
    vw = scene_view(a, image, attached);
    const ReconWalk k = {a.depth, a.depth_type, a.keep, a.thr, scene_seed(a.seed, (uint32_t)image), SCENE_STAGE};
    return recon_lane(k, vw, (uint32_t)vw.h * (uint32_t)vw.w, (uint32_t)tile * RECON_TILE + (uint32_t)tid * RECON_PER_LANE, d, vv, uu);
}

MDRP_GLOBAL __launch_bounds__(RECON_THREADS) void k_scene_count(SceneArgs a, const SceneTransform *__restrict__ T, uint32_t *__restrict__ tcnt) {
    __shared__ uint32_t s_wave[RECON_THREADS / 64];
    const size_t image = blockIdx.x / (uint32_t)a.nt;
    const int tile = (int)(blockIdx.x % (uint32_t)a.nt), tid = threadIdx.x;
    ReconView vw;
    double d[RECON_PER_LANE];
    uint32_t vv[RECON_PER_LANE], uu[RECON_PER_LANE];
    recon_tile_total(scene_lane(a, image, tile, tid, T[image].depth >= 0, vw, d, vv, uu), tid, s_wave, tcnt + blockIdx.x); // (attached: uniform over the workgroup)
}

// The running sums, as k_recon_scan takes its tiles': a thread sums its run of consecutive values, thread 0 scans the run totals, the thread walks its
// run again (a value is read and written by the same thread only).
// phase 0, grid n_images: image blockIdx.x's tile counts in place to their exclusive running sum, its true count to offsets[image + 1].
// phase 1, grid 1: offsets[1 .. n_images] (the counts) in place to their inclusive running sum, offsets[0] = 0: offsets[i] = the rows below image i.
MDRP_GLOBAL __launch_bounds__(RECON_THREADS) void k_scene_scan(int phase, int n_images, int nt, uint32_t *tcnt, int64_t *offsets) {
    __shared__ int64_t s_run[RECON_THREADS];
    const int tid = threadIdx.x, n = phase ? n_images : nt;
    const int per = (n + RECON_THREADS - 1) / RECON_THREADS, lo = min(tid * per, n), hi = min(lo + per, n);
    uint32_t *cnt = tcnt + (size_t)blockIdx.x * (size_t)nt; // (phase 0)
    int64_t sum = 0;
    for (int i = lo; i < hi; ++i) sum += phase ? offsets[(size_t)i + 1] : (int64_t)cnt[i];
    s_run[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int t = 0; t < RECON_THREADS; ++t) {
            const int64_t x = s_run[t];
            s_run[t] = run; // exclusive
            run += x;
        }
        offsets[phase ? 0 : (size_t)blockIdx.x + 1] = phase ? 0 : run;
    }
    __syncthreads();
    int64_t run = s_run[tid];
    if (phase) {
        for (int i = lo; i < hi; ++i) { run += offsets[(size_t)i + 1]; offsets[(size_t)i + 1] = run; }
    } else {
        for (int i = lo; i < hi; ++i) { const uint32_t x = cnt[i]; cnt[i] = (uint32_t)run; run += x; }
    }
}

// Grid: n_images * nt tiles, then the filler workgroups.  (tcnt and offsets are k_scene_scan's.)
MDRP_GLOBAL __launch_bounds__(RECON_THREADS) void k_scene_emit(SceneArgs a, const uint32_t *__restrict__ tcnt, const SceneTransform *__restrict__ T,
                                                              const SceneImage *__restrict__ im, const int64_t *__restrict__ offsets,
                                                              float *__restrict__ points, int32_t *__restrict__ pixel) {
    const uint32_t tiles = (uint32_t)a.n_images * (uint32_t)a.nt; // (fits: the entry point checks the grid)
    const int tid = threadIdx.x;
    const int64_t p_max = a.p_max;
    if (blockIdx.x >= tiles) { // the filler behind the last written row
        const int64_t all = offsets[a.n_images];
        recon_fill((int64_t)(blockIdx.x - tiles) * RECON_TILE, tid, all < p_max ? all : p_max, p_max, points, pixel);
        return;
    }
    __shared__ uint32_t s_wave[RECON_THREADS / 64];
    const size_t image = blockIdx.x / (uint32_t)a.nt;
    const int tile = (int)(blockIdx.x % (uint32_t)a.nt);
    const SceneTransform &t = T[image];
    ReconView vw;
    double d[RECON_PER_LANE];
    uint32_t vv[RECON_PER_LANE], uu[RECON_PER_LANE];
    const unsigned kept = scene_lane(a, image, tile, tid, t.depth >= 0, vw, d, vv, uu);
    const uint32_t before = recon_tile_rank(kept, tid, s_wave);
    if (!kept) return;
    const int64_t row = offsets[image] + (int64_t)tcnt[blockIdx.x] + (int64_t)before;
    const SceneImage &si = im[image];
    const double c0 = a.center ? a.center[2 * image] : 0.0, c1 = a.center ? a.center[2 * image + 1] : 0.0;
    const auto point = [&](uint32_t v, uint32_t u, double dd, double o[3]) { scene_point(t, si, v, u, c0, c1, dd, o); };
    recon_write_rows(kept, row, p_max, vv, uu, d, vw.stride, point, points, pixel);
}

#endif // __HIPCC__

} // namespace mdrp
