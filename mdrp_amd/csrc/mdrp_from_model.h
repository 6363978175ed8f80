// mdrp_from_model.h — refine and verify caller-supplied models (mdrp_refine_batch, include/mdrp.h).
//
// k_from_model<KIND, SHIFT>: one 256-lane workgroup per pair runs what the estimator runs from the moment RANSAC has picked its winner — the
// tail of ransac<> and the wrappers' inlier-only refinement (final_pair) — from a model the CALLER hands in:
//   score the start model | LO (25 it, TRUNCATED, all records), adopted iff it scores better | get_inliers | inlier-only LM | record
// It composes block_score and the two lm_refine forms final_pair uses and restates no arithmetic; the pair states come from k_prep, unchanged.
// A workgroup touches its own pair only: no flags, no waits, no atomics on shared state (the two LM sweep counters of mdrp_stats aside).
// T is fixed at 256 lanes, so a pair's record does not depend on the batch it arrives in, and the loss of the inlier-only refinement is read
// at run time: four instantiations, not k_final's 48.
#pragma once
#include "mdrp_kernels.h"

namespace mdrp {

constexpr int FROM_MODEL_THREADS = 256;
constexpr int STAGE_LO = 1, STAGE_INLIERS = 2; // MDRP_STAGE_* of include/mdrp.h

// the caller's model in the estimator's units: the focal kinds work on coordinates divided by the pair's normalisation scale
template <int KIND>
__device__ __forceinline__ Model from_model_start(const Model *__restrict__ m0, double norm) {
    Model x = *m0;
    if (KIND != 0) { x.f1 /= norm; x.f2 /= norm; }
    return x;
}

template <int KIND, bool SHIFT>
__global__ __launch_bounds__(FROM_MODEL_THREADS, MDRP_LM_MINWAVES) void k_from_model(RunParams rp, const PairState *__restrict__ st, const double *__restrict__ pts,
                                                                                   const double *__restrict__ dep, const Model *__restrict__ models, int stages,
                                                                                   uint8_t *__restrict__ mask_all, ResultDev *__restrict__ results,
                                                                                   double *__restrict__ initial_score /*[batch] or null*/,
                                                                                   int32_t *__restrict__ initial_inliers /*[batch] or null*/, int list_stride,
                                                                                   int mask_index /*1: 3 * list_stride entries of dynamic LDS*/,
                                                                                   unsigned long long *__restrict__ lm_stats) {
    constexpr int T = FROM_MODEL_THREADS;
    extern __shared__ uint16_t lm_dyn_list[];
    __shared__ LmShared sh;
    __shared__ __attribute__((aligned(16))) unsigned int s_ps[(sizeof(PairState) + 3) / 4];
    __shared__ __attribute__((aligned(16))) unsigned int s_m0[sizeof(Model) / 4]; // the caller's model, bit for bit
    __shared__ __attribute__((aligned(16))) double s_logtab[2 * MDRP_LOGTAB_N];
    const int pair = blockIdx.x;
    lm_logtab_load(s_logtab);
    if (threadIdx.x == 0) {
        sh.list = lm_dyn_list; sh.stride = list_stride; sh.midx = mask_index; sh.stats = lm_stats; sh.ev[0] = 0; sh.ev[1] = 0;
        sh.logtab = s_logtab;
    }
    {   // pair state and start model once into LDS: re-readable there, so that only the model under refinement is live across an LM (final_pair)
        const unsigned int *src = reinterpret_cast<const unsigned int *>(st + pair);
        for (int i = threadIdx.x; i < (int)(sizeof(PairState) / 4); i += T) s_ps[i] = src[i];
        const unsigned int *msrc = reinterpret_cast<const unsigned int *>(models + pair);
        for (int i = threadIdx.x; i < (int)(sizeof(Model) / 4); i += T) s_m0[i] = msrc[i];
    }
    __syncthreads();
    const PairState &ps = *reinterpret_cast<const PairState *>(s_ps);
    const Model *m0 = reinterpret_cast<const Model *>(s_m0);
    uint8_t *mask = mask_all + (size_t)pair * rp.n_max;
    if (ps.n < 3) { // (k_prep: n = 0 for a pair of fewer than 3 correspondences) the estimators' rule: zeroed stats, the model as it came
        for (int i = threadIdx.x; i < rp.n_max; i += T) mask[i] = 0;
        if (threadIdx.x == 0) {
            ResultDev res;
            res.model = *m0;
            res.refinements = 0; res.iterations = 0; res.num_inliers = 0; res.inlier_ratio = 0.0; res.model_score = DBL_MAX;
            results[pair] = res;
            if (initial_score) initial_score[pair] = DBL_MAX;
            if (initial_inliers) initial_inliers[pair] = 0;
        }
        return;
    }
    const double *pp = pts + (size_t)pair * rp.n_max * PT_STRIDE;
    const double *dd = dep + (size_t)pair * rp.n_max * 2;
    double *scratch = sh.scratch;
    Model x = from_model_start<KIND>(m0, ps.norm);
    // the start model's own score: the estimator's exact sweep (a NaN model: no inliers, n * sq_thr)
    double score;
    int count;
    block_score<T>(KIND, x, pp, ps.n, ps.sq_thr, scratch, score, count, nullptr);
    if (threadIdx.x == 0) {
        if (initial_score) initial_score[pair] = score;
        if (initial_inliers) initial_inliers[pair] = count;
    }
    int refinements = 0;
    const bool real = x.q[0] == x.q[0];
    if ((stages & STAGE_LO) && real) { // ransac<>'s LO: 25 iterations, TRUNCATED, all records (final_pair's first block)
        LmOpt o;
        o.max_it = 25; o.loss = 1; o.loss_scale = ps.lo_loss_scale;
        o.grad_tol = 1e-10; o.step_tol = 1e-8; o.lambda0 = 1e-3; o.lambda_min = 1e-10; o.lambda_max = 1e10;
        lm_refine<KIND, SHIFT, T, 1>(x, pp, dd, ps.n, nullptr, ps.scale_reproj, rp.weight_sampson, o, sh);
        ++refinements;
        double sc;
        int cn;
        block_score<T>(KIND, x, pp, ps.n, ps.sq_thr, scratch, sc, cn, nullptr);
        if (sc < score) { score = sc; count = cn; }        // adopted WITH its own score (the estimator's record keeps the old one)
        else x = from_model_start<KIND>(m0, ps.norm);      // (re-read: no second model is kept live across the LM)
    }
    {   // get_inliers of the model kept so far
        double sc;
        int cn;
        for (int i = ps.n + threadIdx.x; i < rp.n_max; i += T) mask[i] = 0;
        block_score<T>(KIND, x, pp, ps.n, ps.sq_thr, scratch, sc, cn, mask);
        __syncthreads();
    }
    // the wrappers' inlier-only refinement with the user's BundleOptions (count rule: final_pair)
    if ((stages & STAGE_INLIERS) && count > (KIND == 2 ? 7 : 3)) {
        LmOpt o;
        o.max_it = rp.final_max_it; o.loss = rp.final_loss; o.loss_scale = ps.final_loss_scale;
        o.grad_tol = rp.grad_tol; o.step_tol = rp.step_tol; o.lambda0 = rp.lambda0; o.lambda_min = rp.lambda_min; o.lambda_max = rp.lambda_max;
        lm_refine<KIND, SHIFT, T, -1>(x, pp, dd, ps.n, mask, ps.scale_reproj, rp.weight_sampson, o, sh);
        ++refinements;
    }
    if (KIND != 0) { x.f1 *= ps.norm; x.f2 *= ps.norm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ResultDev res;
        if (refinements) res.model = x;
        else res.model = *m0; // no LM ran (verification, a NaN start): the caller's model, no focal round trip
        res.refinements = (uint64_t)refinements; res.iterations = 0; res.num_inliers = (uint64_t)count;
        res.inlier_ratio = (double)count / (double)ps.n; res.model_score = score;
        results[pair] = res;
        lm_flush_stats(sh);
    }
}

} // namespace mdrp
