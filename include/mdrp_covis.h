/* mdrp_covis.h — part of the C ABI of include/mdrp.h (ABI 0.6): CO-VISIBILITY — how far the two depth maps of a pair agree under the pair's model, as
 * 16 integer counts per pair.  Include mdrp.h, not this file: mdrp.h reaches it through mdrp_dense.h, mdrp_reconstruct.h and the scene header, whose
 * descriptors and rules R1, R3 and R5 it builds on.
 *
 * These entry points are declared here and not in another header because the history matrices of the existing headers enumerate those headers' entry
 * points; the matrix for the entry points of this file is tests/test_gpu_covis_history.py.  A symbol added here needs a call there. */
#ifndef MDRP_COVIS_H
#define MDRP_COVIS_H
#ifndef MDRP_H
#error "include mdrp.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Dense depth-consistency counts (added within ABI 0.6: new symbols only).
 * The only measure of a model so far is the number of sparse matches it was fitted to.  Here a subsample of each image's pixels is carried through
 * the model into the other image and its depth is compared with the depth the other map holds there.  mdrp_amd/frontend.py covisibility_pair_numpy
 * states it in NumPy for one pair, and the device result equals that statement as bytes: every count is an integer, and every quantity that decides
 * one is a fixed sequence of float64 operations, one rounding per arithmetic sign, nothing fused, IEEE division.  For pair b with model m:
 *   C1. usable model.  R1 of mdrp_reconstruct.h.  A pair whose model is not usable has all 16 counters 0; so has, in the per-image form, a pair
 *       with an image index outside the set.  Nothing is read through a bad index.
 *   C2. two directions.  Direction 0 takes image 1's pixels as SOURCES and image 2 as the TARGET; direction 1 is the other way round.  Nothing
 *       depends on the pair's position in the batch.
 *   C3. sources.  Pixel (v, u) of the source's valid region is a candidate by R3's hash with stage = 6 for direction 0 and 7 for direction 1 (1 .. 5
 *       are taken): a smaller thr keeps a subset, and the set does not depend on the subsample of a cloud.  d = (double)depth_src[v][u] is read for a
 *       candidate and for no other pixel.  The pixel is SAMPLED iff d is finite and z = d + shift_src > 0.
 *   C4. the point in the target's frame.  X by R5 (the source's centre, intrinsics and shift).  Direction 0 is R6:
 *           P_r = inv * (((R[r][0] * X0 + R[r][1] * X1) + R[r][2] * X2) + t_r),  inv = 1.0 / scale.
 *       Direction 1 is the inverse, sums left to right:
 *           Y_r = scale * X_r - t_r,   P_r = (R[0][r] * Y0 + R[1][r] * Y1) + R[2][r] * Y2.
 *       The pixel is FRONT iff P2 is finite and P2 > 0.
 *   C5. projection.  xo = P0 / P2, yo = P1 / P2; px = (xo * fx + ox) + c0, py = (yo * fy + oy) + c1 with fx, fy, ox, oy of the TARGET's camera
 *       (MDRP_CALIB) or fx = fy = the model's focal of the target's side and ox = oy = 0 (focal kinds), and (c0, c1) the target image's centre.
 *       R5 takes the integer u for the pixel's own coordinate, so the inverse is the NEAREST pixel: a = px + 0.5, b = py + 0.5, and the pixel is
 *       INSIDE iff a >= 0 && a < w_t && b >= 0 && b < h_t ((h_t, w_t): the target's valid region; a NaN fails).  ut = (int)a, vt = (int)b, by
 *       truncation.
 *   C6. comparison.  dt = (double)depth_tgt[vt][ut], zt = dt + shift_tgt.  The pixel is KNOWN iff dt is finite and zt > 0.  A known pixel is
 *       CONSISTENT iff P2 >= lo * zt && P2 <= hi * zt; OCCLUDED iff P2 > hi * zt (the point lies behind the target's surface); VIOLATING iff
 *       P2 < lo * zt (the point floats in front of a surface the target camera saw: evidence against the model).
 *   C7. output.  counts[b][dir][8] int32: sampled, front, inside, known, consistent, occluded, violating, 0.  Each of the first four classes is a
 *       subset of the one before it, and the last three partition `known`.
 * Every pointer of the descriptors is DEVICE memory. */
enum { MDRP_COVIS_SAMPLED = 0, MDRP_COVIS_FRONT = 1, MDRP_COVIS_INSIDE = 2, MDRP_COVIS_KNOWN = 3, MDRP_COVIS_CONSISTENT = 4, MDRP_COVIS_OCCLUDED = 5,
       MDRP_COVIS_VIOLATING = 6 };  /* the slot of each class */
#define MDRP_COVIS_SLOTS 8          /* counters per direction */

typedef struct {
    uint32_t thr;                  /* 1 .. MDRP_RECON_ALL (R3) */
    int32_t reserved_;
    uint64_t seed;                 /* its low 32 bits are used */
    double lo;                     /* 0 <= lo <= 1: 1.0 - tol, computed by the caller */
    double hi;                     /* 1 <= hi, finite: 1.0 + tol */
} mdrp_covis_opt;                  /* 32 bytes */

/* Queued on the handle's stream; nothing synchronises and nothing crosses to the host.  kind, dp / ip, models_dev, model_stride, cam1_host and
 * cam2_host: as the two-view cloud's entry points of mdrp_reconstruct.h take them.  counts: [batch][2][8] int32 in DEVICE memory.
 * MDRP_ERR_INVALID, before any device work and with the handle left usable: a NULL handle, descriptor or options; a negative batch; a kind outside
 * 0 .. 2; cameras missing for MDRP_CALIB, given for a focal kind, or of a model other than SIMPLE_PINHOLE / PINHOLE; a model_stride below 96 or not a
 * multiple of 8; a depth_type outside its values; thr == 0; lo or hi not finite, or not 0 <= lo <= 1 <= hi; a negative size or n_images; an extent
 * above MDRP_RECON_MAX_EXTENT; a map of 2^31 pixels or more; with batch > 0 a NULL models_dev, counts, pairs or depth map (of a non-empty map); a
 * batch whose tiles do not fit one launch.  batch == 0 succeeds and does nothing. */
int mdrp_covisibility_pairs_async(mdrp_handle *h, int kind, const mdrp_depth_pairs *dp, const mdrp_covis_opt *opt, int batch, const void *models_dev,
                                  int model_stride, const mdrp_camera *cam1_host, const mdrp_camera *cam2_host, int32_t *counts);
int mdrp_covisibility_image_pairs_async(mdrp_handle *h, int kind, const mdrp_depth_image_pairs *ip, const mdrp_covis_opt *opt, int batch,
                                        const void *models_dev, int model_stride, const mdrp_camera *cam1_host, const mdrp_camera *cam2_host,
                                        int32_t *counts);

#ifdef __cplusplus
}
#endif

#include "mdrp_fuse.h" /* the consistency filter of a scene: the scene's cloud gated by rules C5 and C6 against other images of the set */
#endif
