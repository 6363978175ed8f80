// mdrp_prior.h — start each pair's RANSAC from a caller's model (mdrp_estimate_batch_prior, include/mdrp.h).
//
// k_prior<KIND, SHIFT>: one 256-lane workgroup per pair, behind k_prep and before the first solver or sweep reads the pair states, runs prior_stage
// (mdrp_tail.h) for the mono-depth family.  Everything behind it — sampling, retirement against the records, triggers, walk, closing LO, mask,
// inlier-only refinement — is the estimator's, and finds a pair with records where it used to find one without.  A workgroup touches its own pair
// only: no flags, no waits, no atomics on shared state (the two LM sweep counters of mdrp_stats aside).  T is fixed at 256 lanes, so the state a
// prior leaves behind does not depend on the batch it arrives in.
#pragma once
#include "mdrp_tail.h"

namespace mdrp {

constexpr int PRIOR_THREADS = 256;

template <int KIND, bool SHIFT>
__global__ __launch_bounds__(PRIOR_THREADS, MDRP_LM_MINWAVES) void k_prior(RunParams rp, PairState *__restrict__ st, const double *__restrict__ pts,
                                                                         const double *__restrict__ dep, const Model *__restrict__ priors, int list_stride,
                                                                         unsigned long long *__restrict__ lm_stats) {
    constexpr int T = PRIOR_THREADS;
    extern __shared__ uint16_t lm_dyn_list[];
    __shared__ LmShared sh;
    __shared__ __attribute__((aligned(16))) unsigned int s_ps[PAIR_STATE_WORDS];
    __shared__ __attribute__((aligned(16))) unsigned int s_m0[MODEL_WORDS]; // the caller's prior, bit for bit
    const int pair = blockIdx.x;
    if (threadIdx.x == 0) lm_shared_init(sh, lm_dyn_list, list_stride, 0, lm_stats, nullptr);
    stage_pair<T>(s_ps, st + pair, s_m0, priors + pair);
    __syncthreads();
    prior_stage(MonoFam<KIND, SHIFT, T>{rp, pts, dep, sh}, rp, st, *reinterpret_cast<const PairState *>(s_ps), reinterpret_cast<const Model *>(s_m0), pair, 0,
                nullptr);
}

} // namespace mdrp
