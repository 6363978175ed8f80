/* mdrp_reconstruct.h — part of the C ABI of include/mdrp.h (ABI 0.6): the BACK end — models and the pairs' depth maps in, the fused two-view point
 * cloud of every pair out, in camera 2's frame, subsampled, filtered and compacted on the device.  Include mdrp.h, not this file: mdrp.h reaches it
 * through mdrp_dense.h, whose hash (D4) it subsamples with.
 *
 * These entry points are declared here and not in mdrp.h or another extension header because the history matrices of the existing headers enumerate
 * those headers' entry points; the matrix for the entry points of this file is tests/test_gpu_reconstruct_history.py.  A symbol added here needs a
 * call there. */
#ifndef MDRP_RECONSTRUCT_H
#define MDRP_RECONSTRUCT_H
#ifndef MDRP_H
#error "include mdrp.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Fused two-view point clouds (added within ABI 0.6: new symbols only).
 * What the reference's callers do behind the estimator: unproject both depth maps, drop the infinite points, subsample, and bring image 1's cloud into
 * camera 2's frame by the model's own equation R (d1 + shift1) K1^-1 x1 + t = scale (d2 + shift2) K2^-1 x2.  mdrp_amd/frontend.py
 * reconstruct_pair_numpy states it in NumPy for one pair, and the device result equals that statement as bytes.  For pair b with model m:
 *   R1. usable model.  The pair is EMPTY when any of q, t, scale, shift1, shift2 is not finite or scale == 0; for the focal kinds also when f1 or f2
 *       is not finite or is <= 0.  An empty pair has both counts 0 and only filler in its rows.  (MDRP_CALIB's record can be a NaN pose: this is how
 *       it passes through.)
 *   R2. pixel order.  Image 1's pixels in row-major order (v, u), then image 2's.  Nothing depends on the pair's position in the batch.
 *   R3. subsample.  With k = (v << 16) | u and stage = 3 for image 1, 4 for image 2:
 *           hsh = lowbias32((uint32)(seed * 0x9E3779B1 + stage * 0x85EBCA77 + k))        (lowbias32: rule D4 of mdrp_dense.h)
 *       the pixel is a candidate iff thr == MDRP_RECON_ALL or hsh < thr.  A rate r in (0, 1) is thr = floor(r * 2^32); the candidates at a smaller thr
 *       are a subset of those at a larger one.
 *   R4. depth filter.  d = (double)depth[v][u].  MDRP_KEEP_NOT_INF drops the pixel iff d is +-inf (the scripts' rule: a NaN stays);
 *       MDRP_KEEP_FINITE keeps only a finite d.
 *   R5. unprojection, in float64, one rounding per arithmetic sign, nothing fused.  x = (double)u - center[0], y = (double)v - center[1];
 *       MDRP_CALIB: xn = (x - cx) * (1.0 / fx), yn = (y - cy) * (1.0 / fy) with the image's camera; focal kinds: xn = x * (1.0 / f_i),
 *       yn = y * (1.0 / f_i) with f_1 = m.f1, f_2 = m.f2.  z = d + shift_i.  X = (xn * z, yn * z, z).
 *   R6. transform.  Image 2's points are X.  Image 1's are inv * Y with inv = 1.0 / scale and Y_r = ((R[r][0] * X0 + R[r][1] * X1) + R[r][2] * X2) + t_r;
 *       R from q = (w, x, y, z): rows (1 - 2 (yy + zz), 2 (xy - wz), 2 (xz + wy)), (2 (xy + wz), 1 - 2 (xx + zz), 2 (yz - wx)),
 *       (2 (xz - wy), 2 (yz + wx), 1 - 2 (xx + yy)).
 *   R7. output.  Kept points are rounded once to float32 (to nearest) and go in R2's order to rows 0, 1, ... of points[b]; pixel[b][row] = v * w_alloc + u
 *       with w_alloc the ALLOCATED row length of that image's map (w_max in the per-image form): one index gathers the colour.  counts[b] = (n1, n2) are
 *       the TRUE numbers of kept points per image whatever p_max is; rows are written while they fit, image 2's start at min(n1, p_max);
 *       n1 + n2 > p_max says the pair was truncated.  Rows behind the last written one hold 0, 0, 0 and pixel = -1.
 * Every pointer of the descriptors is DEVICE memory. */
enum { MDRP_KEEP_NOT_INF = 0, MDRP_KEEP_FINITE = 1 }; /* keep */
#define MDRP_RECON_MAX_EXTENT 65536                   /* h, w: v and u share the hash's 32-bit key */
#define MDRP_RECON_ALL 0xFFFFFFFFu                    /* thr: every pixel is a candidate */

typedef struct {
    const void *depth1;            /* [B][h1][w1] */
    const void *depth2;            /* [B][h2][w2] */
    int32_t depth_type;            /* MDRP_F32 | MDRP_F64 */
    int32_t h1, w1, h2, w2;        /* 0 .. MDRP_RECON_MAX_EXTENT; a map has fewer than 2^31 pixels */
    int32_t reserved_;
    const double *center1;         /* [B][2] or NULL (the origin) */
    const double *center2;
} mdrp_depth_pairs;                /* 56 bytes */

/* The batch as its producer holds it (mdrp_image_pairs without the keypoints): a map exists once per image, pair b is two indices (a, c) = pairs[b].
 * If a or c is outside [0, n_images) the pair is empty and nothing is read through the bad index.  Otherwise depth1 = depth[a], (h1, w1) = size[a]
 * clamped to [0, h_max] x [0, w_max], center1 = center[a], and the same from c for image 2; the row stride is always w_max. */
typedef struct {
    const void *depth;             /* [I][h_max][w_max] */
    int32_t depth_type;            /* MDRP_F32 | MDRP_F64 */
    int32_t h_max, w_max;          /* 0 .. MDRP_RECON_MAX_EXTENT; h_max * w_max below 2^31 */
    int32_t n_images;              /* I */
    const int32_t *size;           /* [I][2] (h, w) or NULL = the full map */
    const double *center;          /* [I][2] or NULL */
    const int32_t *pairs;          /* [B][2] image indices (a, c) */
} mdrp_depth_image_pairs;          /* 48 bytes */

typedef struct {
    int32_t keep;                  /* MDRP_KEEP_NOT_INF | MDRP_KEEP_FINITE */
    uint32_t thr;                  /* 1 .. MDRP_RECON_ALL */
    uint64_t seed;                 /* its low 32 bits are used */
    int32_t p_max;                 /* rows per pair of points and pixel, >= 0 */
    int32_t reserved_;
} mdrp_reconstruct_opt;            /* 24 bytes */

/* Queued on the handle's stream; nothing synchronises and nothing crosses to the host.  kind: MDRP_CALIB, MDRP_SHARED_FOCAL or MDRP_VARYING_FOCAL.
 * models_dev: [B] records model_stride bytes apart in DEVICE memory, an mdrp_model at the front of each: a stride of 96 is a model array, a stride of
 * 136 is what mdrp_copy_results_device wrote.  cam1_host, cam2_host: [B] cameras in HOST memory, one record per pair — required for MDRP_CALIB, NULL
 * otherwise.  points: [B][p_max][3] floats, pixel: [B][p_max] int32, counts: [B][2] int32, all DEVICE memory.
 * MDRP_ERR_INVALID, before any device work and with the handle left usable: a NULL handle, descriptor or options; a negative batch; a kind outside
 * 0 .. 2; cameras missing for MDRP_CALIB, given for a focal kind, or of a model other than SIMPLE_PINHOLE / PINHOLE; a model_stride below 96 or not a
 * multiple of 8; a depth_type or keep outside its values; thr == 0; p_max < 0; a negative size or n_images; an extent above MDRP_RECON_MAX_EXTENT; a
 * map of 2^31 pixels or more; with batch > 0 a NULL models_dev, counts, pairs, depth map (of a non-empty map), points or pixel (p_max > 0); a batch
 * whose tiles do not fit one launch.  batch == 0 succeeds and does nothing. */
int mdrp_reconstruct_pairs_async(mdrp_handle *h, int kind, const mdrp_depth_pairs *dp, const mdrp_reconstruct_opt *opt, int batch,
                                 const void *models_dev, int model_stride, const mdrp_camera *cam1_host, const mdrp_camera *cam2_host, float *points,
                                 int32_t *pixel, int32_t *counts);
int mdrp_reconstruct_image_pairs_async(mdrp_handle *h, int kind, const mdrp_depth_image_pairs *ip, const mdrp_reconstruct_opt *opt, int batch,
                                       const void *models_dev, int model_stride, const mdrp_camera *cam1_host, const mdrp_camera *cam2_host,
                                       float *points, int32_t *pixel, int32_t *counts);

#ifdef __cplusplus
}
#endif

#include "mdrp_scene.h" /* an image set: the pairs chained along a tree, one fused cloud per scene; it builds on the descriptors and rules above */
#endif
