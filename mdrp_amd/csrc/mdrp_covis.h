// mdrp_covis.h — co-visibility of a pair (include/mdrp_covis.h): how far a pair's two depth maps agree under its model, as 16 integers
// per pair.  One more pass of the back end's tile walk (mdrp_reconstruct.h): a sampled pixel of the source image is unprojected, carried into the
// other camera's frame, projected to the nearest pixel of the target map, and its depth there is compared with the target's own.
//
// mdrp_amd/frontend.py covisibility_pair_numpy is the definition (rules C1-C7).  Every count is an integer; every quantity that decides one is a fixed
// sequence of float64 operations, one rounding per arithmetic sign, none of them fused, IEEE division.  The device result equals the NumPy one as
// bytes.  The first part of this file is host + device arithmetic; the kernels follow behind __HIPCC__:
//   k_covis_pair    a thread per pair: the pair's CovisPair (the ReconPair of mdrp_reconstruct.h, the focals of both sides, the scale) and its 16
//                   counters cleared.  Every word the count kernel reads or adds to is written here, by this call.
//   k_covis_count   a workgroup per tile of RECON_TILE consecutive pixels of one SOURCE image of one pair (image 1: direction 0, image 2: direction 1),
//                   a lane per RECON_PER_LANE consecutive pixels, through recon_side_lane with the stages 6 and 7.  A sampled pixel runs
//                   C4-C6 with one gathered load of the target map; the seven class counts of a wavefront come from ballots and popcounts, and go to
//                   the pair's counters by one integer atomicAdd per wavefront and non-zero class (integer sums do not depend on their order).
// Nothing is proportional to B * h * w: the scratch is the pairs' records and the camera tables.
#pragma once
#include "mdrp_reconstruct.h"

namespace mdrp {

constexpr uint32_t COVIS_STAGE_1 = 6, COVIS_STAGE_2 = 7; // C3: direction 0 | direction 1 (1 and 2: the dense sampler's, 3 and 4: the two-view cloud's, 5: the scene's)
constexpr int COVIS_SLOTS = 8;                           // == MDRP_COVIS_SLOTS: counters per direction
enum : unsigned {                                        // == MDRP_COVIS_*: the slot of each class, and its bit in a pixel's class mask
    COVIS_SAMPLED = 0, COVIS_FRONT = 1, COVIS_INSIDE = 2, COVIS_KNOWN = 3, COVIS_CONSISTENT = 4, COVIS_OCCLUDED = 5, COVIS_VIOLATING = 6, COVIS_CLASSES = 7
};

// what a pixel needs of its pair: written once per pair by k_covis_pair
struct CovisPair {
    ReconPair p;
    double fx[2], fy[2]; // the focal lengths a point is projected with, per side (the camera's, or the model's focal)
    double scale;        // direction 1 multiplies by it (direction 0 by p.inv)
};

// C5's focals of one side, beside recon_side's reciprocals
MDRP_HD void covis_focals(int kind, int id, const double *c, double f, double &fx, double &fy) {
    if (kind == 0) { fx = c[0]; fy = id == 1 ? c[1] : c[0]; }
    else fx = fy = f;
}

MDRP_HD void covis_pair(const double *m, int kind, int id1, const double *cam1, int id2, const double *cam2, CovisPair &cp) {
    recon_pair(m, kind, id1, cam1, id2, cam2, cp.p);
    covis_focals(kind, id1, cam1, m[10], cp.fx[0], cp.fy[0]);
    covis_focals(kind, id2, cam2, m[11], cp.fx[1], cp.fy[1]);
    cp.scale = m[7];
}

// C3's depth test (the source pixel) and C6's (the target pixel): a finite depth in front of its camera
MDRP_HD bool covis_depth_ok(double d, double shift) { return fe_isfinite(d) && d + shift > 0.0; }

// C4: the point of source pixel (v, u) with depth d in the TARGET camera's frame.  dir 0: image 1 -> camera 2, R6 as recon_point states it;
// dir 1: image 2 -> camera 1, the inverse: Y = scale X - t, P = R^T Y, sums left to right.
MDRP_HD void covis_point(const CovisPair &cp, int dir, uint32_t v, uint32_t u, double c0, double c1, double d, double P[3]) {
    if (dir == 0) {
        recon_point(cp.p, 0, v, u, c0, c1, d, P);
        return;
    }
    double X[3], Y[3];
    recon_unproject(cp.p.s[1], v, u, c0, c1, d, X);
    for (int r = 0; r < 3; ++r) Y[r] = recon_mul(cp.scale, X[r]) - cp.p.t[r];
    for (int r = 0; r < 3; ++r) {
        const double a = recon_mul(cp.p.R[r], Y[0]), b = recon_mul(cp.p.R[3 + r], Y[1]), c = recon_mul(cp.p.R[6 + r], Y[2]);
        P[r] = (a + b) + c;
    }
}

// C4's FRONT and C5: the class bits FRONT and INSIDE of a point P in the target's frame, and the target pixel (vt, ut) of an INSIDE one.
// (tc0, tc1): the target image's centre; (ht, wt): its valid region.
MDRP_HD unsigned covis_project(const CovisPair &cp, int dir, const double P[3], double tc0, double tc1, int ht, int wt, uint32_t &vt, uint32_t &ut) {
    const int t = 1 - dir;
    if (!(fe_isfinite(P[2]) && P[2] > 0.0)) return 0;
    const double xo = P[0] / P[2], yo = P[1] / P[2];
    const double px = (recon_mul(xo, cp.fx[t]) + cp.p.s[t].ox) + tc0, py = (recon_mul(yo, cp.fy[t]) + cp.p.s[t].oy) + tc1;
    const double a = px + 0.5, b = py + 0.5; // the nearest pixel: an integer u is the pixel's own coordinate
    if (!(a >= 0.0 && a < (double)wt && b >= 0.0 && b < (double)ht)) return 1u << COVIS_FRONT; // (a NaN fails)
    ut = (uint32_t)(int)a; vt = (uint32_t)(int)b;
    return (1u << COVIS_FRONT) | (1u << COVIS_INSIDE);
}

// C6: the class bits KNOWN and one of CONSISTENT, OCCLUDED, VIOLATING for a point at depth P2 whose target pixel holds dt
MDRP_HD unsigned covis_compare(double P2, double dt, double shift_t, double lo, double hi) {
    if (!covis_depth_ok(dt, shift_t)) return 0;
    const double zt = dt + shift_t;
    const double l = lo * zt, h = hi * zt;
    // three tests as C6 states them: with lo <= hi and zt > 0 exactly one holds (an overflowed zt = inf with lo = 0 makes l a NaN, which fails all of its tests)
    return (1u << COVIS_KNOWN) | ((P2 >= l && P2 <= h) ? 1u << COVIS_CONSISTENT : 0u) | (P2 > h ? 1u << COVIS_OCCLUDED : 0u) | (P2 < l ? 1u << COVIS_VIOLATING : 0u);
}

#if defined(__HIPCC__)

constexpr int COVIS_PAIR_THREADS = 64;

// Grid: ceil(B / COVIS_PAIR_THREADS).  (a: the ReconArgs of the call; its cameras are per pair.)
MDRP_GLOBAL __launch_bounds__(COVIS_PAIR_THREADS) void k_covis_pair(ReconArgs a, int batch, CovisPair *__restrict__ cp, int32_t *__restrict__ counts) {
    const int b = (int)(blockIdx.x * COVIS_PAIR_THREADS + threadIdx.x);
    if (b >= batch) return;
    const ReconCam *c1 = a.kind == 0 ? a.cam1 + b : nullptr, *c2 = a.kind == 0 ? a.cam2 + b : nullptr;
    CovisPair p;
    covis_pair(reinterpret_cast<const double *>(a.models + (size_t)b * (size_t)a.model_stride), a.kind, c1 ? c1->model_id : 0, c1 ? c1->params : nullptr,
               c2 ? c2->model_id : 0, c2 ? c2->params : nullptr, p);
    cp[b] = p;
#pragma unroll
    for (int i = 0; i < 2 * COVIS_SLOTS; ++i) counts[(size_t)b * (2 * COVIS_SLOTS) + i] = 0;
}

// Grid: per pair nt1 tiles of image 1 (direction 0), then nt2 tiles of image 2 (direction 1).  a.keep is RECON_KEEP_FINITE: recon_lane's kept pixels are
// the candidates with a finite depth, and C3 adds the sign test.
MDRP_GLOBAL __launch_bounds__(RECON_THREADS) void k_covis_count(ReconArgs a, const CovisPair *__restrict__ cps, double lo, double hi, int32_t *__restrict__ counts) {
    const int nt = a.nt1 + a.nt2;
    const size_t b = blockIdx.x / (uint32_t)nt;
    const int tile = (int)(blockIdx.x % (uint32_t)nt), tid = threadIdx.x, lane = tid & 63;
    ReconSideTile t;
    double d[RECON_PER_LANE];
    uint32_t vv[RECON_PER_LANE], uu[RECON_PER_LANE];
    const unsigned kept = recon_side_lane(a, b, tile, tid, COVIS_STAGE_1, COVIS_STAGE_2, t, d, vv, uu);
    const int dir = t.side; // (the source image's side is the direction)
    const ReconView tw = recon_view(a, b, 1 - dir);
    const CovisPair &cp = cps[b];
    const double *sc = t.usable ? (dir ? a.center2 : a.center1) : nullptr, *tc = t.usable ? (dir ? a.center1 : a.center2) : nullptr; // (an empty set has no row 0)
    const double c0 = sc ? sc[2 * (size_t)t.vw.image] : 0.0, c1 = sc ? sc[2 * (size_t)t.vw.image + 1] : 0.0;
    const double tc0 = tc ? tc[2 * (size_t)tw.image] : 0.0, tc1 = tc ? tc[2 * (size_t)tw.image + 1] : 0.0;
    const void *tmap = dir ? a.depth1 : a.depth2;
    const double shift_s = cp.p.s[dir].shift, shift_t = cp.p.s[1 - dir].shift;
    unsigned cls[RECON_PER_LANE];
#pragma unroll
    for (int j = 0; j < RECON_PER_LANE; ++j) {
        cls[j] = 0;
        if (!((kept >> j) & 1u) || !(d[j] + shift_s > 0.0)) continue;
        double P[3];
        covis_point(cp, dir, vv[j], uu[j], c0, c1, d[j], P);
        uint32_t vt = 0, ut = 0;
        unsigned c = (1u << COVIS_SAMPLED) | covis_project(cp, dir, P, tc0, tc1, tw.h, tw.w, vt, ut);
        if ((c >> COVIS_INSIDE) & 1u) // (vt < tw.h, ut < tw.w: inside the target's valid region, which lies inside its allocation)
            c |= covis_compare(P[2], dense_ld(tmap, a.depth_type, tw.base + (size_t)vt * (size_t)tw.stride + (size_t)ut), shift_t, lo, hi);
        cls[j] = c;
    }
    // lane k of a wavefront ends up with the wavefront's count of class k
    int mine = 0;
#pragma unroll
    for (int k = 0; k < (int)COVIS_CLASSES; ++k) {
        int n = 0;
#pragma unroll
        for (int j = 0; j < RECON_PER_LANE; ++j) n += __popcll(__ballot((cls[j] >> k) & 1u));
        if (lane == k) mine = n;
    }
    if (lane < (int)COVIS_CLASSES && mine != 0) atomicAdd(counts + (b * 2 + (size_t)dir) * COVIS_SLOTS + lane, mine);
}

#endif // __HIPCC__

} // namespace mdrp
