/* mdrp_classic_models.h — part of the C ABI of include/mdrp.h (ABI 0.6), which includes it: the 5- / 6- / 7-point baselines from a caller's model.
 * Include mdrp.h, not this file.
 *
 * These entry points are declared here and not in mdrp.h or mdrp_classic_ranked.h because tests/history_cases.py and tests/classic_history_cases.py
 * enumerate the handle entry points of those two headers and run each of them behind every other call on one handle; the same matrix for the entry
 * points of this file is tests/test_gpu_classic_models_history.py over tests/classic_models_history_cases.py.  A symbol added here needs a call there. */
#ifndef MDRP_CLASSIC_MODELS_H
#define MDRP_CLASSIC_MODELS_H
#ifndef MDRP_H
#error "include mdrp.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Models of the baselines, in the caller's units (added within ABI 0.6: new symbols only).
 * kind is MDRP_RELPOSE_5PT, MDRP_SHARED_6PT or MDRP_FUNDAMENTAL_7PT (any other kind is MDRP_ERR_INVALID; mdrp_refine_batch and
 * mdrp_estimate_batch_prior keep refusing these three); K is the estimator's sample size 5, 6 or 7.  A model is an mdrp_model as the estimator
 * returns it: the pose q, t (5-point), the pose and f1 = f2 in pixels (6-point), or the fundamental matrix for pixel coordinates, row-major in the
 * first nine doubles of the record (7-point).  A NaN in the record's first double (q[0], F[0]) means "no model" / "no prior".
 * The way into the estimator's units is part of the contract:
 *   5-point: the model as it is; the cameras unproject the points, t is not renormalised.
 *   6-point: f / norm, norm being the pair's normalisation scale.
 *   7-point: with Tinv = [s 0 cx; 0 s cy; 0 0 1] per image (s = norm, c = the image's centroid of the pair's records): M = F Tinv1, then
 *            F_n = Tinv2' M, both products accumulated over the inner index in ascending order.  No rescaling.
 * The way out is the estimator's: F <- T2' F T1 with unit Frobenius norm (7-point), f * norm (6-point). */

/* mdrp_refine_classic — mdrp_refine_batch's list with the baselines' rules.  For pair b with n = n_per_pair[b] records and start model M0:
 *   1. The estimator's normalisation with score_initial_model = 0.  Only max_epipolar_error, the caller's BundleOptions, the cameras (5-point)
 *      and the principal point in cam1 (6-point) are read; every other RansacOptions field is ignored and nothing is refused for it.
 *   2. S0, C0 = MSAC score and inlier count of the converted M0 at the squared threshold: pose scoring with cheirality (5-point), F scoring
 *      (6- and 7-point).  A NaN model scores n * threshold^2 with 0 inliers.
 *   3. MDRP_STAGE_LO, unless M0 is NaN: the estimator's refine_model — 5- and 6-point: the records within 5 threshold^2 of M0, and an LM over them
 *      only if they are more than K; 7-point: an LM over all records; 25 iterations, TRUNCATED loss at the LO's loss scale.  `refinements` counts
 *      the stage whether or not its LM ran.  The result is adopted with its own (S1, C1) iff S1 < S0.
 *   4. mask = get_inliers of the model kept so far; bytes at or past n are 0.
 *   5. MDRP_STAGE_INLIERS, when the count exceeds K: LM over the masked records with the caller's BundleOptions at the final loss scale.
 *   6. Record: the model in the caller's units; model_score, num_inliers, inlier_ratio = count / n and the mask describe the model that ENTERED
 *      stage 5; iterations = 0, refinements = 0..2.  With refinements == 0 the caller's record comes back BIT FOR BIT (no F or focal round
 *      trip).  n < K: the caller's model bit for bit, zeroed stats, model_score = DBL_MAX, a zero mask.
 *   7. initial_score[b] = S0, initial_inliers[b] = C0 (both optional).
 * MDRP_ERR_INVALID, before any device work: another kind, stages outside 0..3, a NULL required buffer, n_per_pair out of range, missing cameras
 * (5-point), a missing principal point (6-point).  A refusal leaves the handle usable.
 * x1, x2, models ([B]) and inlier_mask ([B][n_max] bytes or NULL) live in mem_space; n_per_pair, cameras, out ([B]), initial_score and
 * initial_inliers ([B] each, or NULL) in HOST memory. */
int mdrp_refine_classic(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, int batch, int n_max,
                        const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt,
                        const mdrp_bundle_opt *bopt, const mdrp_model *models, int stages, mdrp_result *out, uint8_t *inlier_mask,
                        double *initial_score, int32_t *initial_inliers);
/* Device-resident variant, as mdrp_refine_batch_async: results through mdrp_fetch_results / mdrp_copy_results_device; the initial_* buffers, when
 * given, are DEVICE memory. */
int mdrp_refine_classic_async(mdrp_handle *h, int kind, const double *x1_dev, const double *x2_dev, int batch, int n_max,
                              const int32_t *n_per_pair_host, const mdrp_camera *cam1_host, const mdrp_camera *cam2_host,
                              const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, const mdrp_model *models_dev, int stages,
                              uint8_t *inlier_mask_dev, double *initial_score_dev, int32_t *initial_inliers_dev);

/* mdrp_estimate_classic_prior — mdrp_estimate_batch for the kind, with every pair of n >= K records whose prior P is not NaN put, behind the
 * normalisation, into the state the search is in after it has scored and LO-refined P as an initial model that was not reset:
 *   - (S0, C0) of P; more = C0 > 0, better = S0 < DBL_MAX.  With neither, no record is set and no LM runs.  Otherwise the records of the minimal
 *     models are C0 and S0, and P is the best model with its score and count.
 *   - one refine_model (as in stage 3 above), refinements = 1, adopted iff it scores below model_score; it never touches the minimal records.
 *   - inlier_ratio and the dynamic iteration bound follow, with the kind's sample size as the exponent.
 *   - not an iteration: iterations stays 0; with max_iterations = 0 the estimator's tail runs on this state.  A pair with a prior ignores
 *     score_initial_model; a pair without one behaves as in mdrp_estimate_batch, that flag included.
 * Everything behind it — sampling, retirement, triggers, walk, closing LO, mask, inlier-only LM, un-normalisation — is the estimator's.
 * prior_space 0: P is in the caller's units and converted as above.  prior_space 1: P is taken as it stands, in the estimator's normalised
 * coordinates (6-point: no focal division; 7-point: no Tinv products; 5-point: identical to 0).  Any other value is MDRP_ERR_INVALID.
 * Refusals are mdrp_estimate_batch's own for the kind (real_focal_check; progressive_sampling: MDRP_ERR_UNSUPPORTED), plus a NULL prior with
 * batch > 0.  x1, x2, prior ([B]) and inlier_mask live in mem_space; n_per_pair, cameras and out in HOST memory.  Host buffers are copied in one
 * piece on the handle's stream (no sliced front).  Iteration budgets and match scores do not combine with priors. */
int mdrp_estimate_classic_prior(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, int batch, int n_max,
                                const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt,
                                const mdrp_bundle_opt *bopt, const mdrp_model *prior, int prior_space, mdrp_result *out, uint8_t *inlier_mask);
/* Device-resident variant, as mdrp_estimate_batch_async. */
int mdrp_estimate_classic_prior_async(mdrp_handle *h, int kind, const double *x1_dev, const double *x2_dev, int batch, int n_max,
                                      const int32_t *n_per_pair_host, const mdrp_camera *cam1_host, const mdrp_camera *cam2_host,
                                      const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, const mdrp_model *prior_dev, int prior_space,
                                      uint8_t *inlier_mask_dev);

#ifdef __cplusplus
}
#endif
#endif
