/* mdrp_classic_focals.h — part of the C ABI of include/mdrp.h (ABI 0.6), which includes it: the varying-focal baseline (`7p` in the reference's
 * tables, /root/reference/eval_varying_f.py:134) — two focal lengths and a pose from the 7-point estimator's fundamental matrix.
 * Include mdrp.h, not this file.
 *
 * These entry points are declared here and not in mdrp.h or another extension header because the history matrices of the existing headers enumerate
 * those headers' entry points; the matrix for the entry points of this file is tests/test_gpu_classic_focals_history.py.  A symbol added here needs
 * a call there. */
#ifndef MDRP_CLASSIC_FOCALS_H
#define MDRP_CLASSIC_FOCALS_H
#ifndef MDRP_H
#error "include mdrp.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Focals and pose from a fundamental matrix (added within ABI 0.6: new symbols only).
 * F is a fundamental matrix for pixel coordinates, x2' F x1 = 0, row-major; pp1, pp2 the principal points of the two images.
 *   1. Focals, the closed form of poselib::focals_from_fundamental (wheel _core.pyi): with p_i = (pp_i, 1), II = diag(1, 1, 0), F e1 = 0, F' e2 = 0,
 *          f1^2 = -(p2' [e2]x II F p1)(p1' F' p2) / (p2' [e2]x II F II F' p2)
 *          f2^2 = -(p1' [e1]x II F' p2)(p2' F p1) / (p1' [e1]x II F' II F p1)
 *      e1 / e2 = the largest of the three cross products of two rows of F / of F' (the first one on ties; no SVD, not normalised: the formula is
 *      homogeneous of degree 0 in them).  f_i = sqrt(f_i^2), NaN where f_i^2 is negative or NaN.
 *   2. E = K2' F K1 with K_i = [f_i 0 ppx_i; 0 f_i ppy_i; 0 0 1], not rescaled.
 *   3. The four poses of motion_from_essential(E) without a cheirality test, in its order: (R1, t), (R1, -t), (R2, -t), (R2, t); t has unit length.
 *   4. Vote: every record i < n of the pair with inlier_mask[i] != 0 (every record, without a mask) is a voter.  Its bearings are
 *      b1 = ((x1 - pp1) / f1, 1), b2 = ((x2 - pp2) / f2, 1), both normalised; votes[c] counts the voters for which check_cheirality(candidate c,
 *      b1, b2, minimum depth 0) holds — the test motion_from_essential applies to its sample points.
 *   5. winner = the candidate with the largest count, the first one on ties.
 * The record: */
typedef struct {
    mdrp_model model;   /* q and unit-length t of the winner; scale = 1, shift1 = shift2 = 0; f1, f2 in pixels */
    int32_t votes[4];
    int32_t voters;
    int32_t winner;
    int32_t status;     /* MDRP_FOCAL_* bits, 0 = a pose chosen by at least one voter */
    int32_t pad_;       /* 0 */
} mdrp_focal_pose;      /* 128 bytes */
enum { MDRP_FOCAL_NO_MODEL = 1,    /* a NaN in F[0] (the estimators' "no model"), or a pair of fewer than 7 records: both focals are NaN */
       MDRP_FOCAL_F1_NOT_REAL = 2, /* f1^2 < 0: f1 is NaN */
       MDRP_FOCAL_F2_NOT_REAL = 4, /* f2^2 < 0: f2 is NaN */
       MDRP_FOCAL_NO_VOTERS = 8 }; /* no record voted (an all-zero mask): winner = 0, the first candidate's pose */
/* With one of the first three bits set nothing is swept: identity pose, winner = -1, votes and voters 0.  MDRP_FOCAL_NO_VOTERS is only ever set alone.
 * A pair's record depends on the pair alone, not on the batch it arrives in or on what the handle ran before. */

/* Step 1 alone for `batch` matrices.  F: [batch][9]; pp1, pp2: [batch][2] or NULL (the origin); f1f2: [batch][2].  All in mem_space.  Synchronous.
 * MDRP_ERR_INVALID: a NULL handle, F or f1f2 with batch > 0, a negative batch, an unknown mem_space. */
int mdrp_focals_from_fundamental(mdrp_handle *h, int mem_space, const double *F, const double *pp1, const double *pp2, int batch, double *f1f2);

/* Steps 1-5 for a batch of pairs.  x1, x2: [batch][n_max][2] pixel coordinates as the caller holds them (rows at or past n_per_pair[b] are never
 * read); n_per_pair: [batch] in HOST memory or NULL (all n_max); models: the F of pair b row-major in the first nine doubles of the record at
 * byte offset b * model_stride_bytes — 96 for packed mdrp_model records (sizeof(mdrp_model)), 136 to point straight at mdrp_result records
 * (sizeof(mdrp_result)); inlier_mask: [batch][n_max] bytes or NULL; pp1, pp2: [batch][2] or NULL (the origin).  x1, x2, models, inlier_mask, pp1
 * and pp2 live in mem_space; out: [batch] records in HOST memory.  Synchronous with respect to `out`.
 * MDRP_ERR_INVALID, before any device work and with the handle left usable: a NULL handle; a negative size; batch > 0 with NULL models or out;
 * batch > 0 and n_max > 0 with NULL x1 or x2; n_per_pair out of range; a model_stride_bytes below 96 or no multiple of 8; an unknown mem_space. */
int mdrp_pose_from_fundamental(mdrp_handle *h, int mem_space, const double *x1, const double *x2, int batch, int n_max, const int32_t *n_per_pair,
                               const void *models, int model_stride_bytes, const uint8_t *inlier_mask, const double *pp1, const double *pp2,
                               mdrp_focal_pose *out);
/* Device-resident variant: every buffer but n_per_pair_host is DEVICE memory, out_dev included ([batch] records of 128 bytes); the kernel is queued
 * on the handle's stream and the call does not wait. */
int mdrp_pose_from_fundamental_async(mdrp_handle *h, const double *x1_dev, const double *x2_dev, int batch, int n_max, const int32_t *n_per_pair_host,
                                     const void *models_dev, int model_stride_bytes, const uint8_t *inlier_mask_dev, const double *pp1_dev,
                                     const double *pp2_dev, mdrp_focal_pose *out_dev);

/* The baseline in one call: mdrp_estimate_batch_async for MDRP_FUNDAMENTAL_7PT (same arguments, same records, same option refusals), then steps 1-5
 * queued behind it on the handle's stream.  The tail reads the estimator's result records (stride 136) and its inlier mask where they lie on the
 * device: nothing returns to the host in between.  inlier_mask_dev: [batch][n_max] bytes or NULL (the handle's own mask is used and not handed out).
 * The 7-point records stay fetchable as after mdrp_estimate_batch_async (mdrp_fetch_results / mdrp_copy_results_device); out_dev is complete once
 * the handle's stream has drained, which either fetch waits for.
 * MDRP_ERR_INVALID, before any device work: a NULL out_dev with batch > 0, and everything mdrp_estimate_batch_async refuses for the kind. */
int mdrp_estimate_fundamental_focals_async(mdrp_handle *h, const double *x1_dev, const double *x2_dev, int batch, int n_max,
                                           const int32_t *n_per_pair_host, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                                           uint8_t *inlier_mask_dev, const double *pp1_dev, const double *pp2_dev, mdrp_focal_pose *out_dev);

#ifdef __cplusplus
}
#endif
#endif
