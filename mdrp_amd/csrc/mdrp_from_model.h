// mdrp_from_model.h — refine and verify caller-supplied models (mdrp_refine_batch, include/mdrp.h).
//
// k_from_model<KIND, SHIFT>: one 256-lane workgroup per pair runs from_model_stage (mdrp_tail.h) for the mono-depth family; the pair states come
// from k_prep, unchanged.  A workgroup touches its own pair only: no flags, no waits, no atomics on shared state (the two LM sweep counters of
// mdrp_stats aside).  T is fixed at 256 lanes, so a pair's record does not depend on the batch it arrives in, and the loss of the inlier-only
// refinement is read at run time: four instantiations, not k_final's 48.
#pragma once
#include "mdrp_tail.h"

namespace mdrp {

constexpr int FROM_MODEL_THREADS = 256;

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
    __shared__ __attribute__((aligned(16))) unsigned int s_ps[PAIR_STATE_WORDS];
    __shared__ __attribute__((aligned(16))) unsigned int s_m0[MODEL_WORDS]; // the caller's model, bit for bit
    __shared__ __attribute__((aligned(16))) double s_logtab[2 * MDRP_LOGTAB_N];
    const int pair = blockIdx.x;
    lm_logtab_load(s_logtab);
    if (threadIdx.x == 0) lm_shared_init(sh, lm_dyn_list, list_stride, mask_index, lm_stats, s_logtab);
    stage_pair<T>(s_ps, st + pair, s_m0, models + pair);
    __syncthreads();
    from_model_stage(MonoFam<KIND, SHIFT, T>{rp, pts, dep, sh}, rp, *reinterpret_cast<const PairState *>(s_ps), reinterpret_cast<const Model *>(s_m0), pair,
                     stages, mask_all, results, initial_score, initial_inliers);
}

} // namespace mdrp
