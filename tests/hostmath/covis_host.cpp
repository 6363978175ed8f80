// Host build of the co-visibility header's arithmetic (mdrp_amd/csrc/mdrp_covis.h: the pair's record, the sampled-pixel rule, the point in the target's
// frame in both directions, the projection to the nearest pixel and the comparison) for tests/test_covis_host.py, which pins it against the NumPy
// definition without a GPU.  Plain C++: g++ fuses nothing on x86-64 without -mfma, which is the rounding the kernels are held to by recon_mul.
#include "../../mdrp_amd/csrc/mdrp_covis.h"

using namespace mdrp;

extern "C" {

void ch_limits(int *out) {
    out[0] = (int)COVIS_STAGE_1; out[1] = (int)COVIS_STAGE_2; out[2] = COVIS_SLOTS; out[3] = (int)COVIS_CLASSES; out[4] = (int)sizeof(CovisPair);
    out[5] = COVIS_SAMPLED; out[6] = COVIS_FRONT; out[7] = COVIS_INSIDE; out[8] = COVIS_KNOWN; out[9] = COVIS_CONSISTENT; out[10] = COVIS_OCCLUDED; out[11] = COVIS_VIOLATING;
}

// One direction of one pair over the whole source map (widened to double by the caller, which is exact): classes[h][w] is the class mask of every
// pixel (0: not sampled), target[h][w][2] the (vt, ut) of an INSIDE one, counts[8] the direction's counters.  c: (c0, c1) of the source, then of the target.
void ch_direction(const double *model, int kind, int id1, const double *cam1, int id2, const double *cam2, int dir, const double *c, int h, int w,
                  const double *src, int ht, int wt, const double *tgt, uint32_t thr, uint32_t seed, double lo, double hi, unsigned char *classes,
                  int32_t *target, int32_t *counts) {
    for (int k = 0; k < COVIS_SLOTS; ++k) counts[k] = 0;
    if (!recon_usable(model, kind)) return;
    CovisPair cp;
    covis_pair(model, kind, id1, cam1, id2, cam2, cp);
    for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u) {
            const size_t at = (size_t)v * w + u;
            classes[at] = 0; target[2 * at] = target[2 * at + 1] = 0;
            if (!recon_candidate(thr, seed, dir ? COVIS_STAGE_2 : COVIS_STAGE_1, (uint32_t)v, (uint32_t)u)) continue;
            const double d = src[at];
            if (!covis_depth_ok(d, cp.p.s[dir].shift)) continue;
            double P[3];
            covis_point(cp, dir, (uint32_t)v, (uint32_t)u, c[0], c[1], d, P);
            uint32_t vt = 0, ut = 0;
            unsigned cls = (1u << COVIS_SAMPLED) | covis_project(cp, dir, P, c[2], c[3], ht, wt, vt, ut);
            if ((cls >> COVIS_INSIDE) & 1u) {
                target[2 * at] = (int32_t)vt; target[2 * at + 1] = (int32_t)ut;
                cls |= covis_compare(P[2], tgt[(size_t)vt * wt + ut], cp.p.s[1 - dir].shift, lo, hi);
            }
            classes[at] = (unsigned char)cls;
            for (int k = 0; k < (int)COVIS_CLASSES; ++k) counts[k] += (int32_t)((cls >> k) & 1u);
        }
}

}
