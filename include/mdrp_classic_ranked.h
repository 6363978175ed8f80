/* mdrp_classic_ranked.h — part of the C ABI of include/mdrp.h (ABI 0.6), which includes it: the 5- / 6- / 7-point baselines in match-score order.
 * Include mdrp.h, not this file.
 *
 * These entry points are declared here and not in mdrp.h because tests/history_cases.py enumerates the handle entry points of mdrp.h itself and
 * runs each of them behind every other call on one handle; the same matrix for the entry points of this file is tests/test_gpu_classic_history.py
 * over tests/classic_history_cases.py.  A symbol added here needs a call there. */
#ifndef MDRP_CLASSIC_RANKED_H
#define MDRP_CLASSIC_RANKED_H
#ifndef MDRP_H
#error "include mdrp.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The 5- / 6- / 7-point baselines in match-score order (added within ABI 0.6: new symbols only).
 * mdrp_estimate_batch_ranked for the comparison rows, which have no depths: kind is MDRP_RELPOSE_5PT, MDRP_SHARED_6PT or MDRP_FUNDAMENTAL_7PT (any
 * other kind is MDRP_ERR_INVALID; mdrp_estimate_batch_ranked keeps refusing these three).  Ranking, sampler, mask order and every other rule are as
 * documented there, with the sample size K = 5 / 6 / 7 of the estimator in the growth table and in the draws: a progressive sample is K - 1 distinct
 * indices from [0, sub-1) and index K-1 := sub-1.  scores == NULL: the records are in quality order already.  max_prosac_iterations <= 1 equals
 * mdrp_estimate_batch on the pre-sorted records bit for bit; a pair with n < K behaves as the plain estimator does.  The calls sample progressively
 * whether ropt->progressive_sampling is 0 or 1, and refuse everything mdrp_estimate_batch refuses for the kind (missing cameras for the 5-point
 * estimator, a missing principal point for the 6-point one, real_focal_check, n_per_pair out of range); a refusal leaves the handle usable.
 * Iteration budgets and priors do not combine with scores.  x1, x2, scores ([B][n_max] doubles or NULL) and inlier_mask live in mem_space;
 * n_per_pair, cameras and out in HOST memory.  Host buffers are copied in one piece on the handle's stream (no sliced front). */
int mdrp_estimate_classic_ranked(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, const double *scores, int batch,
                                 int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2,
                                 const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, mdrp_result *out, uint8_t *inlier_mask);
/* Device-resident variant, as mdrp_estimate_batch_async: results through mdrp_fetch_results / mdrp_copy_results_device. */
int mdrp_estimate_classic_ranked_async(mdrp_handle *h, int kind, const double *x1_dev, const double *x2_dev, const double *scores_dev, int batch,
                                       int n_max, const int32_t *n_per_pair_host, const mdrp_camera *cam1_host, const mdrp_camera *cam2_host,
                                       const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, uint8_t *inlier_mask_dev);
/* Inspection: mdrp_prosac_samples for samples of sample_size records (3, 5, 6 or 7; anything else is MDRP_ERR_INVALID).
 * out: [sum of chunk_lens][sample_size] uint32 in HOST memory; n < sample_size writes nothing.  sample_size 3 is mdrp_prosac_samples. */
int mdrp_prosac_samples_k(mdrp_handle *h, uint64_t seed, int n, int sample_size, uint64_t max_prosac_iterations, const int32_t *chunk_lens,
                          int n_chunks, uint32_t *out);

#ifdef __cplusplus
}
#endif
#endif
