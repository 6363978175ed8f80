/* mdrp_fuse.h — part of the C ABI of include/mdrp.h (ABI 0.6): the CONSISTENCY FILTER of a scene — the fused cloud of an image set with only the
 * points that other images' depth maps confirm, and per point how many do.  Include mdrp.h, not this file: mdrp.h reaches it through mdrp_dense.h,
 * mdrp_reconstruct.h, the scene header and the co-visibility header, whose descriptors and rules (R1, R3-R5, S1-S6, C5, C6) it builds on.
 *
 * This entry point is declared here and not in another header because the history matrices of the existing headers enumerate those headers' entry
 * points; the matrix for the entry point of this file is tests/test_gpu_fuse_history.py.  A symbol added here needs a call there. */
#ifndef MDRP_FUSE_H
#define MDRP_FUSE_H
#ifndef MDRP_H
#error "include mdrp.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Multi-view depth consistency (added within ABI 0.6: new symbols only).
 * The scene's cloud is the raw union of the maps: depth-edge smear, floaters and every surface error of a monocular network are in it, and overlaps
 * appear as contradicting sheets.  Every image of a scene has a transform to its root, so a point of one image can be tested against ANY image of
 * its component: a point stays if at least min_consistent views see a surface at its depth and at most max_violating see through it.
 * mdrp_amd/frontend.py fuse_scene_numpy states it in NumPy, and the device result equals that statement as bytes: all arithmetic is float64, one
 * rounding per arithmetic sign, nothing fused, IEEE division.  With I images, their tree, and views[I][V] (0 <= V <= MDRP_FUSE_MAX_VIEWS):
 *   F1. transforms, candidates, points.  S1-S5 of the scene header, unchanged: the same records, the same hash (stage 5, the per-image seed), the
 *       same depth filter.  For a candidate pixel of an attached image i, X by S5, and Q its point in the root's frame by S6 BEFORE the rounding to
 *       float32 (a root's point is X as it stands).
 *   F2. testable.  The pixel is tested iff its depth d is finite and d + shift_i > 0.  An untested candidate has support (0, 0).
 *   F3. valid view slots.  Slot n = views[i][k] is valid iff 0 <= n < I, n != i, image n is attached (depth >= 0 in its record), root_n == root_i,
 *       and no earlier slot of row i holds the same n.  An invalid slot contributes nothing, and nothing is read through it.  A view need not be a
 *       partner of image i in `pairs`.
 *   F4. the point in view n's camera frame, the inverse of n's record.  A root view: P = Q.  Otherwise
 *           Y_r = s_n * Q_r - t_n[r],   P_r = (R_n[0][r] * Y0 + R_n[1][r] * Y1) + R_n[2][r] * Y2.
 *       The slot is FRONT iff P2 is finite and P2 > 0.
 *   F5. projection and comparison: rules C5 and C6 of the co-visibility header, word for word, with image n as the target - its camera (MDRP_CALIB)
 *       or fx = fy = f_n of its record with ox = oy = 0, its centre, its valid size, shift_n of its record; the nearest pixel by (int)(px + 0.5).
 *       Each valid slot of a tested pixel yields exactly one of: not front, outside, unknown, consistent, occluded, violating.  n_cons and n_viol
 *       count the consistent and the violating slots.
 *   F6. gate and output.  A candidate is kept iff n_cons >= min_consistent && n_viol <= max_violating.  The kept points go out exactly as S6 says:
 *       images in ascending index, an image's pixels row-major, each point rounded once to float32, pixel = v * w_max + u, offsets the TRUE int64
 *       running sums of the kept points whatever p_max is, rows behind the last written one 0, 0, 0 and -1.  support[row] = (n_cons, n_viol) as
 *       two uint8 per written row, 0, 0 behind the last one.  With min_consistent == 0 and max_violating >= V, points, pixel and offsets are byte
 *       for byte the scene cloud's, and support labels every point.  Duplicates of one surface seen by several images are all kept.
 * Every pointer is DEVICE memory unless it is called _host. */
#define MDRP_FUSE_MAX_VIEWS 8

typedef struct {
    int32_t keep;                  /* MDRP_KEEP_NOT_INF | MDRP_KEEP_FINITE (R4) */
    uint32_t thr;                  /* 1 .. MDRP_RECON_ALL (R3) */
    uint64_t seed;                 /* its low 32 bits are used */
    int32_t p_max;                 /* rows of the whole scene */
    int32_t n_views;               /* V: columns of views_dev, 0 .. MDRP_FUSE_MAX_VIEWS */
    double lo;                     /* 0 <= lo <= 1: 1.0 - tol, computed by the caller */
    double hi;                     /* 1 <= hi, finite: 1.0 + tol */
    int32_t min_consistent;        /* >= 0 */
    int32_t max_violating;         /* >= 0 */
} mdrp_fuse_opt;                   /* 48 bytes */

/* Queued on the handle's stream; nothing synchronises and nothing crosses to the host.  kind, ip, batch, models_dev, model_stride, tree_dev and
 * cams_host: as the scene cloud's entry point takes them.  views_dev: [n_images][n_views] int32.  transforms_dev_or_NULL: [n_images] of the 128-byte
 * records of the scene header, written when given.  points: [p_max][3] floats, pixel: [p_max] int32, support: [p_max][2] uint8, offsets:
 * [n_images + 1] int64.
 * MDRP_ERR_INVALID, before any device work and with the handle left usable: everything the scene cloud's entry point refuses (a NULL handle,
 * descriptor or options; a negative batch or n_images; a kind outside 0 .. 2; cameras missing for MDRP_CALIB, given for a focal kind, or of a model
 * other than SIMPLE_PINHOLE / PINHOLE; a model_stride below 96 or not a multiple of 8; a depth_type or keep outside its values; thr == 0; p_max < 0;
 * a negative extent or one above MDRP_RECON_MAX_EXTENT; a map of 2^31 pixels or more; a NULL offsets; with n_images > 0 a NULL tree_dev, pairs or
 * models_dev (batch > 0), depth map (of a non-empty map), points or pixel (p_max > 0); a scene whose tiles do not fit one launch); n_views outside
 * 0 .. MDRP_FUSE_MAX_VIEWS; a NULL views_dev with n_views > 0 and n_images > 0; lo or hi not finite, or not 0 <= lo <= 1 <= hi; a negative
 * min_consistent or max_violating; a NULL support with p_max > 0.  n_images == 0 writes offsets[0] = 0 and the filler. */
int mdrp_fuse_scene_async(mdrp_handle *h, int kind, const mdrp_depth_image_pairs *ip, const mdrp_fuse_opt *opt, int batch, const void *models_dev,
                          int model_stride, const int32_t *tree_dev, const int32_t *views_dev, const mdrp_camera *cams_host,
                          void *transforms_dev_or_NULL, float *points, int32_t *pixel, uint8_t *support, int64_t *offsets);

#ifdef __cplusplus
}
#endif
#endif
