/* mdrp_classic_frontend.h — part of the C ABI of include/mdrp.h (ABI 0.6), which includes it: the device front end of the 5- / 6- / 7-point
 * baselines, straight from a matcher's output WITHOUT depth maps.  Include mdrp.h, not this file.
 *
 * These entry points are declared here and not in mdrp.h, mdrp_classic_ranked.h or mdrp_classic_models.h because the history tables of those three
 * headers (tests/history_cases.py, tests/classic_history_cases.py, tests/classic_models_history_cases.py) enumerate their handle entry points and
 * run each of them behind every other call on one handle; the same matrix for the entry points of this file is
 * tests/test_gpu_classic_frontend_history.py over tests/classic_frontend_history_cases.py.  A symbol added here needs a call there. */
#ifndef MDRP_CLASSIC_FRONTEND_H
#define MDRP_CLASSIC_FRONTEND_H
#ifndef MDRP_H
#error "include mdrp.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Baselines straight from matcher output (added within ABI 0.6: new symbols only).
 * mdrp_matches / mdrp_image_pairs for the comparison rows, which have no depths.  For pair b and match row m = (i, j), in row order:
 *   1. the row is padding and dropped when i < 0 or j < 0, dropped as well when i >= k1 or j >= k2 (rule 1 of mdrp_matches, unchanged);
 *   2. p1 = kp1[b][i], p2 = kp2[b][j], widened to double; the row is dropped unless all four coordinates are finite (the exponent bits are not all
 *      ones: NaN and +-inf go).  There is no map, so no in-map test, and no depth, so no filter;
 *   3. kept rows go, IN MATCH ORDER, to slots s = 0, 1, ...: x1[b][s] = p1 - center1[b] (centres optional, subtracted in double), x2 likewise;
 *      slot[b][m] = s, -1 for a dropped row; n[b] is the number of kept rows; slots >= n[b] hold x = 0.  No depth buffer exists on this path;
 *   4. with scores (one per match row, floats or doubles as score_type says, higher is better) the rules of the ranked front end in mdrp.h apply
 *      unchanged: a score never keeps or drops a row, a kept row is written once at rank(m) = #{m' kept : key(m') > key(m), or key(m') == key(m)
 *      and m' < m} with key = the score as a double, NaN as -inf, -0.0 = +0.0; slot[b][m] is the rank; scores_dev == NULL: the rows are in quality
 *      order already, the unranked gather.
 * Every pointer of the descriptors is DEVICE memory. */
typedef struct {
    const void *kp1, *kp2;           /* [B][k1][2], [B][k2][2] keypoints (x, y) */
    int32_t kp_type;                 /* MDRP_F32 | MDRP_F64 */
    int32_t k1, k2;                  /* keypoints per image */
    const int32_t *matches;          /* [B][m_max][2] index pairs (i into kp1, j into kp2); a negative index marks a padding row */
    int32_t m_max;                   /* match rows per pair */
    const double *center1, *center2; /* [B][2] or NULL */
} mdrp_point_matches;

/* The per-image form: pair b is (a, c) = pairs[b]; kp1 = kp[a], k1 = kp_count[a] clamped to [0, k_max], center1 = center[a], and the same from c
 * for image 2.  An index outside [0, n_images) gives an empty pair (n = 0, every slot -1, x = 0) and nothing is read through it.  a == c and
 * repeated pairs are legal. */
typedef struct {
    const void *kp;                  /* [I][k_max][2] keypoints (x, y) */
    int32_t kp_type;                 /* MDRP_F32 | MDRP_F64 */
    int32_t k_max;                   /* keypoint rows allocated per image */
    const int32_t *kp_count;         /* [I] valid keypoints of each image, clamped to [0, k_max]; NULL = k_max for all */
    const double *center;            /* [I][2] or NULL */
    int32_t n_images;                /* I */
    const int32_t *pairs;            /* [B][2] image indices (a, c) */
    const int32_t *matches;          /* [B][m_max][2] index pairs (i into kp[a], j into kp[c]); a negative index marks a padding row */
    int32_t m_max;                   /* match rows per pair */
} mdrp_point_image_pairs;

/* The front end alone, shaped like mdrp_gather_matches without d1 / d2.  x1, x2: [B][m_max][2], slot: [B][m_max] — DEVICE memory of the caller;
 * n_host: [B] kept rows per pair, HOST memory.  Queued on the handle's stream; returns after the counts have arrived (one stream synchronisation).
 * MDRP_ERR_INVALID, before any device work: a NULL descriptor or output, a negative size or n_images, an unknown kp_type, batch > 0 and m_max > 0
 * with matches (or pairs) NULL, keypoints NULL where their table is not empty; a score_type other than MDRP_F32 / MDRP_F64 with scores_dev != NULL. */
int mdrp_gather_point_matches(mdrp_handle *h, const mdrp_point_matches *pm, int batch, double *x1, double *x2, int32_t *slot, int32_t *n_host);
int mdrp_gather_point_matches_ranked(mdrp_handle *h, const mdrp_point_matches *pm, const void *scores_dev, int score_type, int batch, double *x1,
                                     double *x2, int32_t *slot, int32_t *n_host);
int mdrp_gather_point_image_pairs(mdrp_handle *h, const mdrp_point_image_pairs *pp, int batch, double *x1, double *x2, int32_t *slot,
                                  int32_t *n_host);
int mdrp_gather_point_image_pairs_ranked(mdrp_handle *h, const mdrp_point_image_pairs *pp, const void *scores_dev, int score_type, int batch,
                                         double *x1, double *x2, int32_t *slot, int32_t *n_host);

/* Front end + estimator, shaped like mdrp_estimate_matches_async.  Gathers into buffers of the handle (the ones the monodepth front end uses, minus
 * the depths), copies the B counts to pinned host memory and synchronises the stream ONCE, then runs exactly what mdrp_estimate_batch_async runs on
 * (x1, x2, d1 = d2 = NULL, n_max = m_max, n_per_pair = the counts); the ranked forms run what mdrp_estimate_classic_ranked_async runs with
 * scores == NULL on the ranked gather: the progressive sampler, whether ropt->progressive_sampling is 0 or 1.  Results through mdrp_fetch_results /
 * mdrp_copy_results_device.  kind: MDRP_RELPOSE_5PT, MDRP_SHARED_6PT or MDRP_FUNDAMENTAL_7PT (any other kind is MDRP_ERR_INVALID;
 * mdrp_estimate_matches_async and its siblings keep refusing these three).  Cameras stay one record per pair in HOST memory, as the baselines take
 * them: cameras for the 5-point estimator, the principal point in cam1 for the 6-point one.  match_mask_dev: [B][m_max] bytes in DEVICE memory or
 * NULL — 1 where the row was kept and is an inlier; n_used_host: [B] in HOST memory or NULL — the counts.
 * Refused before any device work: the descriptor errors above, and the estimator's own refusals (missing cameras or principal point,
 * real_focal_check; progressive_sampling on the unranked forms: MDRP_ERR_UNSUPPORTED).  A refusal leaves the handle usable.  Iteration budgets and
 * priors do not combine with this front end. */
int mdrp_estimate_classic_matches_async(mdrp_handle *h, int kind, const mdrp_point_matches *pm, int batch, const mdrp_camera *cam1_host,
                                        const mdrp_camera *cam2_host, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                                        uint8_t *match_mask_dev, int32_t *n_used_host);
int mdrp_estimate_classic_matches_ranked_async(mdrp_handle *h, int kind, const mdrp_point_matches *pm, const void *scores_dev, int score_type,
                                               int batch, const mdrp_camera *cam1_host, const mdrp_camera *cam2_host, const mdrp_ransac_opt *ropt,
                                               const mdrp_bundle_opt *bopt, uint8_t *match_mask_dev, int32_t *n_used_host);
int mdrp_estimate_classic_image_pairs_async(mdrp_handle *h, int kind, const mdrp_point_image_pairs *pp, int batch, const mdrp_camera *cam1_host,
                                            const mdrp_camera *cam2_host, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                                            uint8_t *match_mask_dev, int32_t *n_used_host);
int mdrp_estimate_classic_image_pairs_ranked_async(mdrp_handle *h, int kind, const mdrp_point_image_pairs *pp, const void *scores_dev,
                                                   int score_type, int batch, const mdrp_camera *cam1_host, const mdrp_camera *cam2_host,
                                                   const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, uint8_t *match_mask_dev,
                                                   int32_t *n_used_host);

#ifdef __cplusplus
}
#endif
#endif
