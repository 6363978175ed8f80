// mdrp_prior.h — start each pair's RANSAC from a caller's model (mdrp_estimate_batch_prior, include/mdrp.h).
//
// k_prior<KIND, SHIFT>: one 256-lane workgroup per pair, behind k_prep and before the first solver or sweep reads the pair states, puts the pair
// into the state ransac<> is in after it has scored and LO-refined an initial model that was NOT reset to the identity (score_initial_model with
// *best = the prior):
//   score the prior | records (best_min_cnt, best_min_score) | best model | LO (25 it, TRUNCATED, all records), adopted iff it scores better |
//   inlier ratio and dynamic iteration bound
// Not an iteration: `iterations` stays 0 and no stop test runs.  Everything behind it — sampling, retirement against the records, triggers, walk,
// closing LO, mask, inlier-only refinement — is the estimator's, and finds a pair with records where it used to find one without.
// It composes block_score, lm_refine (as k_lo compiles it) and dyn_max_iter_of and restates no arithmetic.  A workgroup touches its own pair only:
// no flags, no waits, no atomics on shared state (the two LM sweep counters of mdrp_stats aside).  T is fixed at 256 lanes, so the state a prior
// leaves behind does not depend on the batch it arrives in.  Pairs of fewer than 3 correspondences and pairs whose prior has a NaN q[0] (no prior)
// keep what k_prep gave them, RansacOptions::score_initial_model included; a pair WITH a prior ignores that switch.
#pragma once
#include "mdrp_from_model.h"

namespace mdrp {

constexpr int PRIOR_THREADS = 256;

template <int KIND, bool SHIFT>
__global__ __launch_bounds__(PRIOR_THREADS, MDRP_LM_MINWAVES) void k_prior(RunParams rp, PairState *__restrict__ st, const double *__restrict__ pts,
                                                                         const double *__restrict__ dep, const Model *__restrict__ priors, int list_stride,
                                                                         unsigned long long *__restrict__ lm_stats) {
    constexpr int T = PRIOR_THREADS;
    extern __shared__ uint16_t lm_dyn_list[];
    __shared__ LmShared sh;
    __shared__ __attribute__((aligned(16))) unsigned int s_ps[(sizeof(PairState) + 3) / 4];
    __shared__ __attribute__((aligned(16))) unsigned int s_m0[sizeof(Model) / 4]; // the caller's prior, bit for bit
    const int pair = blockIdx.x;
    if (threadIdx.x == 0) { sh.list = lm_dyn_list; sh.stride = list_stride; sh.midx = 0; sh.stats = lm_stats; sh.ev[0] = 0; sh.ev[1] = 0; sh.logtab = nullptr; }
    {   // pair state and prior once into LDS (k_from_model): only the model under refinement is live across the LM
        const unsigned int *src = reinterpret_cast<const unsigned int *>(st + pair);
        for (int i = threadIdx.x; i < (int)(sizeof(PairState) / 4); i += T) s_ps[i] = src[i];
        const unsigned int *msrc = reinterpret_cast<const unsigned int *>(priors + pair);
        for (int i = threadIdx.x; i < (int)(sizeof(Model) / 4); i += T) s_m0[i] = msrc[i];
    }
    __syncthreads();
    const PairState &ps = *reinterpret_cast<const PairState *>(s_ps);
    const Model *m0 = reinterpret_cast<const Model *>(s_m0);
    if (ps.n < 3 || !(m0->q[0] == m0->q[0])) return; // (uniform: read from LDS)  no search / no prior: k_prep's state stands
    const double *pp = pts + (size_t)pair * rp.n_max * PT_STRIDE;
    const double *dd = dep + (size_t)pair * rp.n_max * 2;
    Model x = from_model_start<KIND>(m0, ps.norm);
    // score_models<> on {prior} against the empty records (0 inliers, DBL_MAX)
    double s0;
    int c0;
    block_score<T>(KIND, x, pp, ps.n, ps.sq_thr, sh.scratch, s0, c0, nullptr);
    const bool more = c0 > 0, better = s0 < DBL_MAX;
    double score = DBL_MAX; // model_score of the run
    int count = 0;
    if (s0 < score) { score = s0; count = c0; }
    int refinements = 0;
    bool adopted = false;
    if (more || better) { // (neither: a NaN score — no record, no LO)
        LmOpt o;
        o.max_it = 25; o.loss = 1; o.loss_scale = ps.lo_loss_scale;
        o.grad_tol = 1e-10; o.step_tol = 1e-8; o.lambda0 = 1e-3; o.lambda_min = 1e-10; o.lambda_max = 1e10;
        lm_refine<KIND, SHIFT, T, 1>(x, pp, dd, ps.n, nullptr, ps.scale_reproj, rp.weight_sampson, o, sh);
        refinements = 1;
        double s1;
        int c1;
        block_score<T>(KIND, x, pp, ps.n, ps.sq_thr, sh.scratch, s1, c1, nullptr);
        if (s1 < score) { score = s1; count = c1; adopted = true; }
    }
    if (threadIdx.x == 0) {
        PairState &d = st[pair];
        // the LO never touches the records of the minimal models
        d.best_min_cnt = more ? (uint64_t)c0 : 0;
        d.best_min_score = better ? s0 : DBL_MAX;
        d.model_score = score;
        d.num_inliers = (uint64_t)count;
        d.best = adopted ? x : from_model_start<KIND>(m0, ps.norm); // (*best = the prior from the start: it stays where nothing beats DBL_MAX)
        d.refinements = (uint64_t)refinements;
        const double ratio = refinements ? (double)count / (double)ps.n : 0.0;
        d.inlier_ratio = ratio;
        d.dyn_max_iter = refinements ? dyn_max_iter_of(rp, ratio) : rp.max_iterations;
        lm_flush_stats(sh);
    }
}

} // namespace mdrp
