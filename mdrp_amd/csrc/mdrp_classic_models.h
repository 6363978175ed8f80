// mdrp_classic_models.h — the 5- / 6- / 7-point baselines from a caller's model (include/mdrp_classic_models.h):
//   kc_from_model<CK>   refine and verify (mdrp_refine_classic): k_from_model's list (mdrp_from_model.h) with the baselines' rules
//   kc_prior<CK>        start the search from it (mdrp_estimate_classic_prior): k_prior's state (mdrp_prior.h) behind kc_prep
// One 256-lane workgroup per pair.  Both compose cblock_score, clm_lo, clm_refine and classic_unnormalize (mdrp_classic.h) and restate no
// arithmetic; the pair states come from kc_prep, unchanged.  A workgroup touches its own pair only: no flags, no waits, no atomics on shared
// state.  T is fixed at 256 lanes, so a pair's record does not depend on the batch it arrives in.  Pairs of fewer records than the sample size
// (kc_prep: n = 0) and pairs whose model has a NaN first double (no model) return before any record is read.
#pragma once
#include "mdrp_classic.h"
#include "mdrp_from_model.h"

namespace mdrp {

constexpr int CLASSIC_MODEL_THREADS = 256;

// The caller's model in the estimator's units (the way in; classic_unnormalize is the way out).
//   5-point: as it is (the cameras unproject the points; t is not renormalised)
//   6-point: f / norm
//   7-point: F_n = T2^-T (F T1^-1) with T^-1 = [s 0 cx; 0 s cy; 0 0 1] per image, s = norm: classic_unnormalize's loops on the inverse
//            transforms, no rescaling
// space 1: the record is in the estimator's normalised coordinates already and is taken as it stands.
template <int CK>
__device__ __forceinline__ Model classic_model_start(const Model *__restrict__ m0, const PairState &ps, int space) {
    Model x = *m0;
    if (space != 0) return x;
    if (CK == CLASSIC_SHARED) { x.f1 /= ps.norm; x.f2 /= ps.norm; }
    if (CK == CLASSIC_FUND) {
        double *F = model_F(x);
        const double s = ps.norm;
        const double T1[9] = {s, 0, ps.cen[0], 0, s, ps.cen[1], 0, 0, 1}, T2[9] = {s, 0, ps.cen[2], 0, s, ps.cen[3], 0, 0, 1};
        double M[9], O[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) M[3 * i + j] = F[3 * i] * T1[j] + F[3 * i + 1] * T1[3 + j] + F[3 * i + 2] * T1[6 + j];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) O[3 * i + j] = T2[i] * M[j] + T2[3 + i] * M[3 + j] + T2[6 + i] * M[6 + j];
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = O[i];
    }
    return x;
}

template <int CK>
__global__ __launch_bounds__(CLASSIC_MODEL_THREADS, 2) void kc_from_model(RunParams rp, const PairState *__restrict__ st, const double *__restrict__ pts,
                                                                         const Model *__restrict__ models, int stages, uint8_t *__restrict__ mask_all,
                                                                         ResultDev *__restrict__ results, double *__restrict__ initial_score /*[batch] or null*/,
                                                                         int32_t *__restrict__ initial_inliers /*[batch] or null*/,
                                                                         int list_stride /*2 * list_stride u16 of dynamic LDS, or 0*/) {
    constexpr int T = CLASSIC_MODEL_THREADS, K = ClassicTraits<CK>::K;
    extern __shared__ uint16_t clm_dyn_list[];
    __shared__ double scratch[4 * MAX_ACC];
    __shared__ ClmList cl;
    __shared__ __attribute__((aligned(16))) unsigned int s_ps[(sizeof(PairState) + 3) / 4];
    __shared__ __attribute__((aligned(16))) unsigned int s_m0[sizeof(Model) / 4]; // the caller's model, bit for bit
    const int pair = blockIdx.x;
    if (threadIdx.x == 0) { cl.list = clm_dyn_list; cl.stride = list_stride; }
    {   // pair state and start model once into LDS (k_from_model): only the model under refinement is live across an LM
        const unsigned int *src = reinterpret_cast<const unsigned int *>(st + pair);
        for (int i = threadIdx.x; i < (int)(sizeof(PairState) / 4); i += T) s_ps[i] = src[i];
        const unsigned int *msrc = reinterpret_cast<const unsigned int *>(models + pair);
        for (int i = threadIdx.x; i < (int)(sizeof(Model) / 4); i += T) s_m0[i] = msrc[i];
    }
    __syncthreads();
    const PairState &ps = *reinterpret_cast<const PairState *>(s_ps);
    const Model *m0 = reinterpret_cast<const Model *>(s_m0);
    uint8_t *mask = mask_all + (size_t)pair * rp.n_max;
    const bool real = m0->q[0] == m0->q[0];
    if (ps.n < K || !real) { // (uniform: read from LDS)  the estimators' rule for n < K: zeroed stats, the model as it came; a NaN model has no inliers
        for (int i = threadIdx.x; i < rp.n_max; i += T) mask[i] = 0;
        if (threadIdx.x == 0) {
            const double s0 = ps.n < K ? DBL_MAX : ps.sq_thr * (double)ps.n;
            ResultDev res;
            res.model = *m0;
            res.refinements = 0; res.iterations = 0; res.num_inliers = 0; res.inlier_ratio = 0.0; res.model_score = s0;
            results[pair] = res;
            if (initial_score) initial_score[pair] = s0;
            if (initial_inliers) initial_inliers[pair] = 0;
        }
        return;
    }
    const double *pp = pts + (size_t)pair * rp.n_max * PT_STRIDE;
    Model x = classic_model_start<CK>(m0, ps, 0);
    double score;
    int count;
    cblock_score<CK, T>(x, pp, ps.n, ps.sq_thr, scratch, score, count, nullptr);
    if (threadIdx.x == 0) {
        if (initial_score) initial_score[pair] = score;
        if (initial_inliers) initial_inliers[pair] = count;
    }
    for (int i = ps.n + threadIdx.x; i < rp.n_max; i += T) mask[i] = 0;
    int refinements = 0;
    if (stages & STAGE_LO) { // the estimator's refine_model; counted whether or not its LM ran, adopted with its own score
        clm_lo<CK, T>(x, ps, pp, mask, scratch, cl); // the output mask doubles as the LO's subset mask (cfinal_pair)
        ++refinements;
        double sc;
        int cn;
        cblock_score<CK, T>(x, pp, ps.n, ps.sq_thr, scratch, sc, cn, nullptr);
        if (sc < score) { score = sc; count = cn; }
        else x = classic_model_start<CK>(m0, ps, 0); // (re-read: no second model is kept live across the LM)
    }
    {   // get_inliers of the model kept so far
        double sc;
        int cn;
        cblock_score<CK, T>(x, pp, ps.n, ps.sq_thr, scratch, sc, cn, mask);
    }
    if ((stages & STAGE_INLIERS) && count > K) { // the estimator's inlier-only refinement with the caller's BundleOptions (cfinal_pair)
        LmOpt f;
        f.max_it = rp.final_max_it; f.loss = rp.final_loss; f.loss_scale = ps.final_loss_scale;
        f.grad_tol = rp.grad_tol; f.step_tol = rp.step_tol; f.lambda0 = rp.lambda0; f.lambda_min = rp.lambda_min; f.lambda_max = rp.lambda_max;
        clm_refine<CK, T>(x, pp, ps.n, mask, f, scratch, cl);
        ++refinements;
    }
    classic_unnormalize<CK>(x, ps);
    if (threadIdx.x == 0) {
        ResultDev res;
        if (refinements) res.model = x;
        else res.model = *m0; // no stage ran (verification): the caller's record, no F or focal round trip
        res.refinements = (uint64_t)refinements; res.iterations = 0; res.num_inliers = (uint64_t)count;
        res.inlier_ratio = (double)count / (double)ps.n; res.model_score = score;
        results[pair] = res;
    }
}

template <int CK>
__global__ __launch_bounds__(CLASSIC_MODEL_THREADS, 2) void kc_prior(RunParams rp, PairState *__restrict__ st, const double *__restrict__ pts,
                                                                    const Model *__restrict__ priors, int prior_space,
                                                                    uint8_t *__restrict__ lo_mask /*[batch][n_max]: clm_lo's subset mask*/,
                                                                    int list_stride /*2 * list_stride u16 of dynamic LDS, or 0*/) {
    constexpr int T = CLASSIC_MODEL_THREADS, K = ClassicTraits<CK>::K;
    extern __shared__ uint16_t clm_dyn_list[];
    __shared__ double scratch[4 * MAX_ACC];
    __shared__ ClmList cl;
    __shared__ __attribute__((aligned(16))) unsigned int s_ps[(sizeof(PairState) + 3) / 4];
    __shared__ __attribute__((aligned(16))) unsigned int s_m0[sizeof(Model) / 4]; // the caller's prior, bit for bit
    const int pair = blockIdx.x;
    if (threadIdx.x == 0) { cl.list = clm_dyn_list; cl.stride = list_stride; }
    {
        const unsigned int *src = reinterpret_cast<const unsigned int *>(st + pair);
        for (int i = threadIdx.x; i < (int)(sizeof(PairState) / 4); i += T) s_ps[i] = src[i];
        const unsigned int *msrc = reinterpret_cast<const unsigned int *>(priors + pair);
        for (int i = threadIdx.x; i < (int)(sizeof(Model) / 4); i += T) s_m0[i] = msrc[i];
    }
    __syncthreads();
    const PairState &ps = *reinterpret_cast<const PairState *>(s_ps);
    const Model *m0 = reinterpret_cast<const Model *>(s_m0);
    if (ps.n < K || !(m0->q[0] == m0->q[0])) return; // (uniform: read from LDS)  no search / no prior: kc_prep's state stands
    const double *pp = pts + (size_t)pair * rp.n_max * PT_STRIDE;
    Model x = classic_model_start<CK>(m0, ps, prior_space);
    // score_models<> on {prior} against the empty records (0 inliers, DBL_MAX)
    double s0;
    int c0;
    cblock_score<CK, T>(x, pp, ps.n, ps.sq_thr, scratch, s0, c0, nullptr);
    const bool more = c0 > 0, better = s0 < DBL_MAX;
    double score = DBL_MAX; // model_score of the run
    int count = 0;
    if (s0 < score) { score = s0; count = c0; }
    int refinements = 0;
    bool adopted = false;
    if (more || better) { // (neither: a NaN score — no record, no LO)
        clm_lo<CK, T>(x, ps, pp, lo_mask + (size_t)pair * rp.n_max, scratch, cl);
        refinements = 1;
        double s1;
        int c1;
        cblock_score<CK, T>(x, pp, ps.n, ps.sq_thr, scratch, s1, c1, nullptr);
        if (s1 < score) { score = s1; count = c1; adopted = true; }
    }
    if (threadIdx.x == 0) {
        PairState &d = st[pair];
        // the LO never touches the records of the minimal models
        d.best_min_cnt = more ? (uint64_t)c0 : 0;
        d.best_min_score = better ? s0 : DBL_MAX;
        d.model_score = score;
        d.num_inliers = (uint64_t)count;
        d.best = adopted ? x : classic_model_start<CK>(m0, ps, prior_space); // (*best = the prior from the start)
        d.refinements = (uint64_t)refinements;
        const double ratio = refinements ? (double)count / (double)ps.n : 0.0;
        d.inlier_ratio = ratio;
        d.dyn_max_iter = refinements ? dyn_max_iter_of(rp, ratio) : rp.max_iterations;
        d.iterations = 0; // not an iteration
    }
}

} // namespace mdrp
