// mdrp_classic_models.h — the 5- / 6- / 7-point baselines from a caller's model (include/mdrp_classic_models.h):
//   kc_from_model<CK>   refine and verify (mdrp_refine_classic): from_model_stage (mdrp_tail.h) for the baselines
//   kc_prior<CK>        start the search from it (mdrp_estimate_classic_prior): prior_stage (mdrp_tail.h) behind kc_prep
// One 256-lane workgroup per pair; the pair states come from kc_prep, unchanged.  A workgroup touches its own pair only: no flags, no waits, no
// atomics on shared state.  T is fixed at 256 lanes, so a pair's record does not depend on the batch it arrives in.  Pairs of fewer records than
// the sample size (kc_prep: n = 0) and pairs whose model has a NaN first double (no model) return before any record is read.
#pragma once
#include "mdrp_classic.h"

namespace mdrp {

constexpr int CLASSIC_MODEL_THREADS = 256;

template <int CK>
__global__ __launch_bounds__(CLASSIC_MODEL_THREADS, 2) void kc_from_model(RunParams rp, const PairState *__restrict__ st, const double *__restrict__ pts,
                                                                         const Model *__restrict__ models, int stages, uint8_t *__restrict__ mask_all,
                                                                         ResultDev *__restrict__ results, double *__restrict__ initial_score /*[batch] or null*/,
                                                                         int32_t *__restrict__ initial_inliers /*[batch] or null*/,
                                                                         int list_stride /*2 * list_stride u16 of dynamic LDS, or 0*/) {
    constexpr int T = CLASSIC_MODEL_THREADS;
    extern __shared__ uint16_t clm_dyn_list[];
    __shared__ ClmShared sh;
    __shared__ __attribute__((aligned(16))) unsigned int s_ps[PAIR_STATE_WORDS];
    __shared__ __attribute__((aligned(16))) unsigned int s_m0[MODEL_WORDS]; // the caller's model, bit for bit
    const int pair = blockIdx.x;
    if (threadIdx.x == 0) { sh.cl.list = clm_dyn_list; sh.cl.stride = list_stride; }
    stage_pair<T>(s_ps, st + pair, s_m0, models + pair);
    __syncthreads();
    const PairState &ps = *reinterpret_cast<const PairState *>(s_ps);
    const Model *m0 = reinterpret_cast<const Model *>(s_m0);
    if (ps.n >= ClassicTraits<CK>::K && !(m0->q[0] == m0->q[0])) { // (uniform: read from LDS)  the baselines' rule for a NaN model: no inliers, nothing runs
        from_model_empty<T>(rp, pair, m0, ps.sq_thr * (double)ps.n, mask_all, results, initial_score, initial_inliers);
        return;
    }
    from_model_stage(ClassicFam<CK, T>{rp, pts, sh}, rp, ps, m0, pair, stages, mask_all, results, initial_score, initial_inliers);
}

template <int CK>
__global__ __launch_bounds__(CLASSIC_MODEL_THREADS, 2) void kc_prior(RunParams rp, PairState *__restrict__ st, const double *__restrict__ pts,
                                                                    const Model *__restrict__ priors, int prior_space,
                                                                    uint8_t *__restrict__ lo_mask /*[batch][n_max]: clm_lo's subset mask*/,
                                                                    int list_stride /*2 * list_stride u16 of dynamic LDS, or 0*/) {
    constexpr int T = CLASSIC_MODEL_THREADS;
    extern __shared__ uint16_t clm_dyn_list[];
    __shared__ ClmShared sh;
    __shared__ __attribute__((aligned(16))) unsigned int s_ps[PAIR_STATE_WORDS];
    __shared__ __attribute__((aligned(16))) unsigned int s_m0[MODEL_WORDS]; // the caller's prior, bit for bit
    const int pair = blockIdx.x;
    if (threadIdx.x == 0) { sh.cl.list = clm_dyn_list; sh.cl.stride = list_stride; }
    stage_pair<T>(s_ps, st + pair, s_m0, priors + pair);
    __syncthreads();
    prior_stage(ClassicFam<CK, T>{rp, pts, sh}, rp, st, *reinterpret_cast<const PairState *>(s_ps), reinterpret_cast<const Model *>(s_m0), pair, prior_space,
                lo_mask + (size_t)pair * rp.n_max);
}

} // namespace mdrp
