// mdrp_tu.hip - one of the library's secondary translation units: compiled once per group with -DMDRP_TU=<group> (mdrp_amd/build.py),
// it holds the explicit instantiations of that group's kernels (mdrp_instances.h) and nothing else.  No host code, no state.
#define MDRP_SECONDARY_TU 1
#include "mdrp_kernels.h"
#include "mdrp_classic.h"
#include "mdrp_from_model.h"
#include "mdrp_prior.h"
#include "mdrp_prosac.h"
#include "mdrp_classic_models.h"
#define MDRP_INST
#include "mdrp_instances.h"
namespace mdrp {
#if MDRP_TU == 1
MDRP_INSTANCES_FINAL_64
#elif MDRP_TU == 2
MDRP_INSTANCES_FINAL_256
#elif MDRP_TU == 3
MDRP_INSTANCES_CLASSIC
#elif MDRP_TU == 4
MDRP_INSTANCES_FROM_MODEL
#elif MDRP_TU == 5
MDRP_INSTANCES_PRIOR
#elif MDRP_TU == 6
MDRP_INSTANCES_CLASSIC_MODELS
#else
#error "MDRP_TU must be 1 (k_final, 64 lanes), 2 (k_final, 256 lanes), 3 (5- / 6- / 7-point baselines), 4 (k_from_model), 5 (k_prior) or 6 (kc_from_model, kc_prior)"
#endif
} // namespace mdrp
