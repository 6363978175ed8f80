/* mdrp_scene.h — part of the C ABI of include/mdrp.h (ABI 0.6): the back end for an IMAGE SET — the pairs' models chained along a tree, and one
 * fused point cloud per scene: every image unprojected once, in the frame of its root.  Include mdrp.h, not this file: mdrp.h reaches it through
 * mdrp_dense.h and mdrp_reconstruct.h, whose descriptors, options and rules R1, R3-R5 it builds on.
 *
 * These entry points are declared here and not in mdrp_reconstruct.h or another header because the history matrices of the existing headers enumerate
 * those headers' entry points; the matrix for the entry points of this file is tests/test_gpu_scene_history.py.  A symbol added here needs a call
 * there. */
#ifndef MDRP_SCENE_H
#define MDRP_SCENE_H
#ifndef MDRP_H
#error "include mdrp.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Scenes (added within ABI 0.6: new symbols only).
 * The reference's video demo carries every frame to its first anchor's frame by R' = R_anchor R, t' = R_anchor t + scale t_anchor,
 * s' = s_anchor scale; a per-image batch (mdrp_image_pairs) wants the same along a spanning tree of its pairs.  mdrp_amd/frontend.py
 * scene_transforms_numpy and reconstruct_scene_numpy state it in NumPy, and the device result equals that statement as bytes.  With I images, B
 * pairs (a, c) = pairs[b] and their models:
 *   S1. tree.  tree[i] = (pair, role) says where image i hangs.  role MDRP_SCENE_ABSENT (0): the image is not part of the scene.  role
 *       MDRP_SCENE_EDGE (1): it hangs on the OTHER image of pairs[pair] = (a, c).  If i == a the edge is the model itself, X_c = (R X_a + t) / scale:
 *       (R_e, t_e, s_e) = (R, t, scale) with R from q by R6 of mdrp_reconstruct.h, and the image's own shift and focal are shift1 and f1.  If i == c
 *       the edge is the inverse, X_a = (R^T X_c - (R^T t) inv) / inv with inv = 1.0 / scale: R_e = R^T, t_e[r] = -(((R[0][r] t[0] + R[1][r] t[1]) +
 *       R[2][r] t[2]) * inv), s_e = inv, and the image's own are shift2 and f2.  role MDRP_SCENE_ROOT (2): the identity; shift and focal from the
 *       image's side of pairs[pair]; pair == -1 is allowed for MDRP_CALIB only, with shift 0.  MDRP_CALIB records f = 0 (its focals are the cameras').
 *       An image is DETACHED when its role is none of the three, when (pair != -1 or not a calibrated root) pair is outside [0, B), a == c, i is
 *       neither a nor c, the other index is outside [0, I), or the pair's model is not usable by R1 of mdrp_reconstruct.h (a root with a pair is held
 *       to all of this too).  A detached or absent image emits nothing, and so does every image whose way to a root passes one.  Nothing is read
 *       through a bad index.
 *   S2. accumulation, leaf upward, in float64, every product and every sum rounded on its own (no fused multiply-add).  acc = image i's own edge,
 *       depth = 1 (a root: the identity, depth = 0, root = i).  Then, with n the other image of the last edge, at most I times: if n is absent or
 *       detached by S1, i is detached; if n is a root, root = n and the walk ends; otherwise with e = n's edge
 *           R'[r][c] = (R_e[r][0] R[0][c] + R_e[r][1] R[1][c]) + R_e[r][2] R[2][c]
 *           t'[r]    = ((R_e[r][0] t[0] + R_e[r][1] t[1]) + R_e[r][2] t[2]) + s t_e[r]
 *           s'       = s s_e
 *       depth += 1, and n = the other image of e.  A walk that has not met a root after I steps (a cycle) leaves i detached.  The record of a
 *       detached or absent image is zeros with root = depth = -1.  With forward edges only this is the video demo's rule composed from the leaf's
 *       end; the two agree up to rounding.
 *   S3. subsample: R3 with stage = 5 and, in the seed's place, seed_i = lowbias32((uint32)(seed + 0xC2B2AE35 * (i + 1))): the kept set of an image
 *       depends on (seed, i, v, u) alone, and a smaller thr keeps a subset.
 *   S4. depth filter: R4.
 *   S5. unprojection: R5 with z = d + shift_i and, for the focal kinds, the image's own f of S1; MDRP_CALIB: the image's camera.
 *   S6. output.  A root's point is X as it stands; any other image's is out[r] = (((R[r][0] X0 + R[r][1] X1) + R[r][2] X2) + t[r]) * inv_s with
 *       inv_s = 1.0 / s of its record: the frame of its root.  Images in ascending index, an image's kept pixels row-major; each point rounded once
 *       to float32; pixel = v * w_max + u.  offsets[i] is the TRUE exclusive running sum of the kept points of the images below i (int64,
 *       offsets[I] the scene's) whatever p_max is; a point goes to row offsets[i] + its place in the image while that is below p_max, so
 *       offsets[I] > p_max says the scene was truncated.  Rows behind the last written one hold 0, 0, 0 and pixel = -1.  A forest is allowed:
 *       every component is in its own root's frame, and `root` of the record says which.
 * Every pointer is DEVICE memory unless it is called _host. */
enum { MDRP_SCENE_ABSENT = 0, MDRP_SCENE_EDGE = 1, MDRP_SCENE_ROOT = 2 }; /* tree[i][1] */

typedef struct {
    double R[9];                   /* row-major */
    double t[3];
    double s;                      /* a point X of the image is (R X + t) * (1.0 / s) in the frame of `root` */
    double f;                      /* the image's own focal (focal kinds; 0 for MDRP_CALIB) */
    double shift;                  /* the image's own depth shift */
    int32_t root;                  /* the image whose frame this is, -1 = absent or detached */
    int32_t depth;                 /* edges to the root, -1 = absent or detached */
} mdrp_scene_transform;            /* 128 bytes */

/* Queued on the handle's stream; nothing synchronises and nothing crosses to the host.  kind, models_dev, model_stride: as
 * mdrp_reconstruct_pairs_async.  pairs_dev: [batch][2] int32, tree_dev: [n_images][2] int32 (pair, role), transforms_dev: [n_images] records.
 * MDRP_ERR_INVALID, before any device work and with the handle left usable: a NULL handle; a negative batch or n_images; a kind outside 0 .. 2; a
 * model_stride below 96 or not a multiple of 8; with n_images > 0 a NULL tree_dev or transforms_dev; with n_images > 0 and batch > 0 a NULL
 * models_dev or pairs_dev.  n_images == 0 succeeds and does nothing; batch == 0 is a scene of pair-less roots and detached images. */
int mdrp_scene_transforms_async(mdrp_handle *h, int kind, int batch, const void *models_dev, int model_stride, const int32_t *pairs_dev,
                                int n_images, const int32_t *tree_dev, mdrp_scene_transform *transforms_dev);

/* The same chaining, then the fused cloud of the whole image set by S3-S6.  ip: one map per image, size, center, pairs (mdrp_depth_image_pairs);
 * opt: mdrp_reconstruct_opt with p_max the rows of the whole SCENE.  cams_host: [n_images] cameras in HOST memory, one per IMAGE - required for
 * MDRP_CALIB, NULL otherwise.  transforms_dev_or_NULL: [n_images] records, written when given.  points: [p_max][3] floats, pixel: [p_max] int32,
 * offsets: [n_images + 1] int64.
 * MDRP_ERR_INVALID, before any device work and with the handle left usable: a NULL handle, descriptor or options; a negative batch or n_images; a
 * kind outside 0 .. 2; cameras missing for MDRP_CALIB (n_images > 0), given for a focal kind, or of a model other than SIMPLE_PINHOLE / PINHOLE; a
 * model_stride below 96 or not a multiple of 8; a depth_type or keep outside its values; thr == 0; p_max < 0; a negative extent or one above
 * MDRP_RECON_MAX_EXTENT; a map of 2^31 pixels or more; a NULL offsets; with n_images > 0 a NULL tree_dev, pairs (batch > 0), models_dev (batch > 0),
 * depth map (of a non-empty map), points or pixel (p_max > 0); a scene whose tiles (1024 pixels each, at least one per image, plus p_max / 1024) do
 * not fit one launch of 2^31 - 1 workgroups - the tile indexing needs no tighter limit on the scene's pixels.  n_images == 0 writes offsets[0] = 0
 * and the filler. */
int mdrp_reconstruct_scene_async(mdrp_handle *h, int kind, const mdrp_depth_image_pairs *ip, const mdrp_reconstruct_opt *opt, int batch,
                                 const void *models_dev, int model_stride, const int32_t *tree_dev, const mdrp_camera *cams_host,
                                 mdrp_scene_transform *transforms_dev_or_NULL, float *points, int32_t *pixel, int64_t *offsets);

#ifdef __cplusplus
}
#endif

#include "mdrp_covis.h" /* co-visibility: dense depth-consistency counts per pair; it builds on the descriptors and rules of mdrp_reconstruct.h */
#endif
