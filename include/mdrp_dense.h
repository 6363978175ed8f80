/* mdrp_dense.h — part of the C ABI of include/mdrp.h (ABI 0.6), which includes it: the front end for DENSE matchers — a warp, its certainty and
 * two depth maps in, the monodepth estimators' records out, sampled by certainty on the device.  Include mdrp.h, not this file.
 *
 * These entry points are declared here and not in mdrp.h or another extension header because the history matrices of the existing headers enumerate
 * those headers' entry points; the matrix for the entry points of this file is tests/test_gpu_dense_history.py.  A symbol added here needs a call
 * there. */
#ifndef MDRP_DENSE_H
#define MDRP_DENSE_H
#ifndef MDRP_H
#error "include mdrp.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Sample a dense warp by certainty (added within ABI 0.6: new symbols only).
 * mdrp_amd/frontend.py sample_dense_numpy states the sampler in NumPy for one pair; every quantity that decides a pick is an integer, and the device
 * result equals that statement as bytes.  For pair b, warp row r = (xA, yA, xB, yB) with certainty c = (double)certainty[r]:
 *   D1. pixel coordinates in float64 on the widened value.  MDRP_DENSE_NORMALIZED: px = (x + 1.0) * (0.5 * W), py = (y + 1.0) * (0.5 * H) with the size
 *       of the row's own image; MDRP_DENSE_PIXEL: the value as it is.
 *   D2. the row is a candidate iff rules 2-4 of mdrp_matches hold for its two points (inside the maps, pixel = truncation, the depth filter) and c is
 *       finite and > 0.  A map without pixels has no candidate.
 *   D3. weight q = 0 for a non-candidate, else min(65536, max(1, floor(c' * 65536.0))) with c' = 1.0 if c > threshold else c.  T = sum q (64 bits),
 *       K = candidates.
 *   D4. the stratified draw of M from integer weights w_0 .. w_{L-1} of sum S > 0, for a stage and the seed: for k = 0 .. M-1,
 *           u_k = lowbias32((uint32)(seed * 0x9E3779B1 + stage * 0x85EBCA77 + k)) >> 8
 *           lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (uint32)
 *           P_k = (k * S + ((u_k * S) >> 24)) / M                                                          (uint64)
 *           pick_k = the smallest i whose inclusive running sum exceeds P_k.
 *       Picks do not decrease with k; a pick equal to its predecessor is dropped.  The hash never takes the pair's position in the batch: a pair's
 *       result does not depend on the batch it arrives in.
 *   D5. stage 1: M1 = min(expansion * n, K) (expansion = 1 without balancing), D4 on q with stage = 1: m1 <= M1 distinct rows, ascending.  T = 0: the
 *       pair is empty.
 *   D6. stage 2 (balanced != 0): a stage-1 pick's cell is (xi1 * grid / W1, yi1 * grid / H1, xi2 * grid / W2, yi2 * grid / H2) in integers, count =
 *       the stage-1 picks in its cell (itself included), w = (1 << 20) / count if count >= min_count else 1; M2 = min(n, m1), D4 on w with stage = 2:
 *       the final rows, ascending.  (An isolated match is almost never kept.)  Without balancing the stage-1 picks are the final rows.
 *   D7. for the final rows in ascending row order: x1 = p1 - center1, x2 = p2 - center2, d1, d2 in float64; rows[j] = the warp row of record j and
 *       score[j] = its widened certainty; behind the count x = 0, d = 1, rows = -1, score = 0.  ranked != 0: the records leave in descending order of
 *       the certainty instead, ties by ascending row (rule 6 of the ranked front end: the order "presorted" records have).
 * The defaults of threshold (0.05), expansion (4), grid (8) and min_count (2) are untuned: their effect on pose accuracy has not been measured.
 * Every pointer is DEVICE memory. */
enum { MDRP_DENSE_NORMALIZED = 0, MDRP_DENSE_PIXEL = 1 }; /* coords */
#define MDRP_DENSE_MAX_ROWS (1 << 22)   /* rows */
#define MDRP_DENSE_MAX_STAGE1 65536     /* expansion * n */
#define MDRP_DENSE_MAX_N 16384          /* n */
#define MDRP_DENSE_MAX_GRID 8           /* grid */
typedef struct {
    const void *warp;              /* [B][rows][4] floats or doubles, contiguous ((B, Hc, Wc, 4) is rows = Hc * Wc) */
    int32_t warp_type;             /* MDRP_F32 | MDRP_F64 */
    int32_t rows;                  /* 0 .. MDRP_DENSE_MAX_ROWS */
    const void *certainty;         /* [B][rows] */
    int32_t certainty_type;        /* MDRP_F32 | MDRP_F64 */
    int32_t coords;                /* MDRP_DENSE_NORMALIZED | MDRP_DENSE_PIXEL */
    const void *depth1;            /* [B][h1][w1] */
    const void *depth2;            /* [B][h2][w2] */
    int32_t depth_type;            /* MDRP_F32 | MDRP_F64 */
    int32_t h1, w1, h2, w2;        /* the images' sizes: each map has its image's size */
    int32_t filter;                /* MDRP_FILTER_BOTH_INF | MDRP_FILTER_FINITE */
    const double *center1;         /* [B][2] or NULL (the origin) */
    const double *center2;
    int32_t n;                     /* records wanted per pair, 1 .. MDRP_DENSE_MAX_N */
    int32_t balanced;              /* 0: stage 1 alone */
    int32_t expansion;             /* >= 1, expansion * n <= MDRP_DENSE_MAX_STAGE1 */
    int32_t grid;                  /* 1 .. MDRP_DENSE_MAX_GRID */
    int32_t min_count;             /* >= 1 */
    int32_t ranked;                /* 0: ascending row order; otherwise descending certainty */
    uint64_t seed;                 /* its low 32 bits are used */
    double threshold;
    int32_t *rows_out;             /* mdrp_estimate_dense_async only, may be NULL: [B][n], the warp row of every record, -1 behind the count */
    double *score_out;             /* mdrp_estimate_dense_async only, may be NULL: [B][n], the certainty of every record */
} mdrp_dense_matches;              /* 144 bytes */

/* The sampler alone into the caller's device buffers.  x1, x2: [B][n][2]; d1, d2, score: [B][n] doubles; rows: [B][n] int32; n_host: [B] counts in
 * HOST memory, written behind the call's one stream synchronisation.  desc->rows_out and desc->score_out are not looked at.
 * MDRP_ERR_INVALID, before any device work and with the handle left usable: a NULL handle, descriptor or output; a negative batch; with batch > 0
 * a NULL warp or certainty (rows > 0) or depth map (of a non-empty map); a type, coords or filter outside its values; a negative size; rows, n or
 * expansion * n outside their limits; grid outside 1 .. 8; expansion < 1; min_count < 1. */
int mdrp_sample_dense(mdrp_handle *h, const mdrp_dense_matches *desc, int batch, double *x1, double *x2, double *d1, double *d2, int32_t *rows,
                      double *score, int32_t *n_host);

/* The sampler, then the monodepth estimator of `kind` (MDRP_CALIB, MDRP_SHARED_FOCAL, MDRP_VARYING_FOCAL) on the handle's stream: what
 * mdrp_estimate_batch_async computes on mdrp_sample_dense's buffers with n_max = n and n_per_pair = the counts, byte for byte.  The records go to
 * buffers of the handle; the counts cross to the host behind one stream synchronisation (n_used_host: [B] or NULL).  record_mask_dev: [B][n] bytes
 * or NULL, the inlier mask per sampled record; desc->rows_out maps a record back to its warp row.  The result records are fetched as after
 * mdrp_estimate_batch_async.  With desc->ranked the records are in descending certainty and the progressive sampler draws from them, whether
 * ropt->progressive_sampling is 0 or 1 (mdrp_estimate_batch_ranked_async with scores_dev = NULL); without desc->ranked progressive_sampling is
 * refused as on every unranked entry point.
 * MDRP_ERR_INVALID, before any device work: everything mdrp_sample_dense refuses of the descriptor, a kind outside 0 .. 2, NULL options, and the
 * estimator's own refusals (taken with progressive_sampling cleared when desc->ranked). */
int mdrp_estimate_dense_async(mdrp_handle *h, int kind, const mdrp_dense_matches *desc, int batch, const mdrp_camera *cam1_host,
                              const mdrp_camera *cam2_host, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, uint8_t *record_mask_dev,
                              int32_t *n_used_host);

#ifdef __cplusplus
}
#endif

#include "mdrp_reconstruct.h" /* the back end: fused two-view point clouds from models and depth maps; it subsamples with D4's hash */
#endif
