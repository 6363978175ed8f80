// Host build of the back end's arithmetic (mdrp_amd/csrc/mdrp_reconstruct.h: the hash, the depth filter, the usable-model rule, the pair's record and
// the point of a kept pixel) for tests/test_reconstruct_host.py, which pins it against the NumPy definition without a GPU.  Plain C++: g++ fuses
// nothing on x86-64 without -mfma, which is the rounding the kernels are held to by recon_mul.
#include "../../mdrp_amd/csrc/mdrp_reconstruct.h"

using namespace mdrp;

extern "C" {

void rh_limits(int *out) { out[0] = RECON_KEEP_NOT_INF; out[1] = RECON_KEEP_FINITE; out[2] = RECON_MAX_EXTENT; out[3] = (int)RECON_STAGE_1; out[4] = (int)RECON_STAGE_2; out[5] = RECON_MODEL_BYTES; }

void rh_hash(uint32_t seed, uint32_t stage, int n, const uint32_t *v, const uint32_t *u, uint32_t *out) {
    for (int i = 0; i < n; ++i) out[i] = recon_hash(seed, stage, v[i], u[i]);
}

int rh_candidate(uint32_t thr, uint32_t seed, uint32_t stage, uint32_t v, uint32_t u) { return recon_candidate(thr, seed, stage, v, u) ? 1 : 0; }

int rh_keep(double d, int keep) { return recon_keep(d, keep) ? 1 : 0; }

int rh_usable(const double *model, int kind) { return recon_usable(model, kind) ? 1 : 0; }

// n pixels (v, u) with depths d of image `side` of one pair: out[n][3] float, the rounded points
void rh_points(const double *model, int kind, int id1, const double *cam1, int id2, const double *cam2, int side, double c0, double c1, int n, const uint32_t *v,
               const uint32_t *u, const double *d, float *out) {
    ReconPair p;
    recon_pair(model, kind, id1, cam1, id2, cam2, p);
    for (int i = 0; i < n; ++i) {
        double o[3];
        recon_point(p, side, v[i], u[i], c0, c1, d[i], o);
        out[3 * i] = (float)o[0]; out[3 * i + 1] = (float)o[1]; out[3 * i + 2] = (float)o[2];
    }
}

}
