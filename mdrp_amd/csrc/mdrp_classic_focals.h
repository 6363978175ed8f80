// mdrp_classic_focals.h — the varying-focal baseline's tail (include/mdrp_classic_focals.h): from the 7-point estimator's fundamental
// matrix to two focal lengths and a pose.
//   focals_from_F        f1, f2 from F and the two principal points: poselib::focals_from_fundamental's closed form (Bougnoux), with the epipoles taken
//                        as the largest cross product of two rows of F' / F — no SVD, not normalised (the formula is homogeneous of degree 0 in them)
//   essential_from_F     E = K2' F K1, K_i = [f_i 0 ppx_i; 0 f_i ppy_i; 0 0 1], not rescaled
//   focal_pose_head      both, then motion_from_essential_emit (mdrp_classic_math.h) with npts = 0: the four candidates in its order,
//                        (R1, t), (R1, -t), (R2, -t), (R2, t), and the status bits of the record
//   focal_pose_votes     the cheirality test of one record against the four candidates
//   focal_pose_record    votes -> winner -> the 128-byte record
// The first part compiles for host and device (MDRP_HD), so that tests/hostmath/focals_host.cpp can pin it on the CPU; the kernels behind it are
// device code: kc_focals (one lane per matrix) and kc_focal_pose (one 256-lane workgroup per pair: the closed form once, then a strided sweep of
// the pair's records with four integer counters per lane).  A workgroup touches its own pair only: no atomics, no state between workgroups.
#pragma once
#include "mdrp_classic_math.h"

namespace mdrp {

struct FocalPose { // == mdrp_focal_pose
    Model model;
    int32_t votes[4];
    int32_t voters, winner, status, pad_;
};
static_assert(sizeof(FocalPose) == 128, "mdrp_focal_pose is 128 bytes");

enum { FOCAL_NO_MODEL = 1, FOCAL_F1_NOT_REAL = 2, FOCAL_F2_NOT_REAL = 4, FOCAL_NO_VOTERS = 8 };
constexpr int FOCAL_MIN_RECORDS = 7; // the 7-point estimator returns no model for fewer
constexpr int FOCAL_POSE_THREADS = 256;

// the null vector of the 3 x 3 matrix with rows r0, r1, r2 of rank 2: the largest of the three cross products of two rows (the first one on ties)
MDRP_HD void focal_null_vector(const double *r0, const double *r1, const double *r2, double *e) {
    double c01[3], c02[3], c12[3];
    cross3(r0, r1, c01); cross3(r0, r2, c02); cross3(r1, r2, c12);
    const double n01 = dot3(c01, c01), n02 = dot3(c02, c02), n12 = dot3(c12, c12);
    double best = n01;
    e[0] = c01[0]; e[1] = c01[1]; e[2] = c01[2];
    if (n02 > best) { best = n02; e[0] = c02[0]; e[1] = c02[1]; e[2] = c02[2]; }
    if (n12 > best) { e[0] = c12[0]; e[1] = c12[1]; e[2] = c12[2]; }
}

// f_a^2 = -(pb' [eb]x II M pa)(pb' M pa) / (pb' [eb]x II M II M' pb) with II = diag(1, 1, 0), M' eb = 0:
// M = F, (pa, pb, eb) = (p1, p2, e2) gives f1^2; M = F', (p2, p1, e1) gives f2^2
MDRP_HD double focal_squared(const double M[9], const double pa[3], const double pb[3], const double eb[3]) {
    double v[3], u[3], z[3], w[3];
    for (int i = 0; i < 3; ++i) v[i] = M[3 * i] * pa[0] + M[3 * i + 1] * pa[1] + M[3 * i + 2] * pa[2];
    const double s = dot3(pb, v);                                                                         // pb' M pa
    v[2] = 0.0;
    cross3(eb, v, w);
    const double num = dot3(pb, w);                                                                       // pb' [eb]x II M pa
    for (int j = 0; j < 3; ++j) u[j] = M[j] * pb[0] + M[3 + j] * pb[1] + M[6 + j] * pb[2];                // M' pb
    u[2] = 0.0;
    for (int i = 0; i < 3; ++i) z[i] = M[3 * i] * u[0] + M[3 * i + 1] * u[1] + M[3 * i + 2] * u[2];       // M II M' pb
    z[2] = 0.0;
    cross3(eb, z, w);
    const double den = dot3(pb, w);
    return -(num * s) / den;
}

MDRP_HD double focal_real_root(double fsq) { return fsq >= 0.0 ? sqrt(fsq) : (double)NAN; } // a negative (or NaN) square has no real focal length

MDRP_HD void focals_from_F(const double F[9] /*row-major*/, const double pp1[2], const double pp2[2], double &f1, double &f2) {
    const double Ft[9] = {F[0], F[3], F[6], F[1], F[4], F[7], F[2], F[5], F[8]};
    const double p1[3] = {pp1[0], pp1[1], 1.0}, p2[3] = {pp2[0], pp2[1], 1.0};
    double e1[3], e2[3];
    focal_null_vector(F, F + 3, F + 6, e1);    // F e1 = 0
    focal_null_vector(Ft, Ft + 3, Ft + 6, e2); // F' e2 = 0
    f1 = focal_real_root(focal_squared(F, p1, p2, e2));
    f2 = focal_real_root(focal_squared(Ft, p2, p1, e1));
}

MDRP_HD void essential_from_F(const double F[9], double f1, double f2, const double pp1[2], const double pp2[2], double E[9]) {
    double M[9]; // F K1
    for (int i = 0; i < 3; ++i) {
        M[3 * i] = F[3 * i] * f1;
        M[3 * i + 1] = F[3 * i + 1] * f1;
        M[3 * i + 2] = F[3 * i] * pp1[0] + F[3 * i + 1] * pp1[1] + F[3 * i + 2];
    }
    for (int j = 0; j < 3; ++j) { // K2' M
        E[j] = f2 * M[j];
        E[3 + j] = f2 * M[3 + j];
        E[6 + j] = pp2[0] * M[j] + pp2[1] * M[3 + j] + M[6 + j];
    }
}

// what the workgroup shares: the closed-form part of a pair
struct FocalPoseHead {
    double f1, f2;
    Model cand[4];
    int32_t status, n_cand;
};

MDRP_HD void focal_pose_head(const double F[9], int n, const double pp1[2], const double pp2[2], FocalPoseHead &hd) {
    hd.status = 0; hd.n_cand = 0;
    hd.f1 = hd.f2 = (double)NAN;
    for (int c = 0; c < 4; ++c) model_identity(hd.cand[c]);
    if (!(F[0] == F[0]) || n < FOCAL_MIN_RECORDS) { hd.status = FOCAL_NO_MODEL; return; }
    focals_from_F(F, pp1, pp2, hd.f1, hd.f2);
    if (!(hd.f1 == hd.f1)) hd.status |= FOCAL_F1_NOT_REAL;
    if (!(hd.f2 == hd.f2)) hd.status |= FOCAL_F2_NOT_REAL;
    if (hd.status) return;
    double E[9];
    essential_from_F(F, hd.f1, hd.f2, pp1, pp2, E);
    int k = 0;
    Model *cand = hd.cand;
    motion_from_essential_emit(E, (const double (*)[3])nullptr, (const double (*)[3])nullptr, 0, [&](const Model &m) { if (k < 4) cand[k] = m; ++k; });
    hd.n_cand = k;
}

// the candidates as the sweep reads them: R1, R2 and t (candidates 0 and 2 carry them; 1 and 3 are the same rotations with the translation negated)
struct FocalPoseFrame {
    double R1[9], R2[9], t[3]; // (candidate 3's translation is candidate 0's, bit for bit)
    double f1, f2, pp1[2], pp2[2];
};
MDRP_HD void focal_pose_frame(const FocalPoseHead &hd, const double pp1[2], const double pp2[2], FocalPoseFrame &fr) {
    quat_to_R(hd.cand[0].q, fr.R1);
    quat_to_R(hd.cand[2].q, fr.R2);
    for (int k = 0; k < 3; ++k) fr.t[k] = hd.cand[0].t[k];
    fr.f1 = hd.f1; fr.f2 = hd.f2;
    fr.pp1[0] = pp1[0]; fr.pp1[1] = pp1[1]; fr.pp2[0] = pp2[0]; fr.pp2[1] = pp2[1];
}

// check_cheirality @0x1dce00 on unit bearings (cheirality_bearing, mdrp_classic_math.h), with the two depths handed out: under t -> -t both change
// sign exactly (a does not depend on t), so one evaluation per rotation decides two candidates
MDRP_HD void focal_cheirality_depths(const double R[9], const double t[3], const double x1[3], const double x2[3], double &l1, double &l2) {
    const double u0 = R[0] * x1[0] + R[1] * x1[1] + R[2] * x1[2], u1 = R[3] * x1[0] + R[4] * x1[1] + R[5] * x1[2],
                 u2 = R[6] * x1[0] + R[7] * x1[1] + R[8] * x1[2];
    const double a = -(u0 * x2[0] + u1 * x2[1] + u2 * x2[2]);
    const double b1 = -(u0 * t[0] + u1 * t[1] + u2 * t[2]);
    const double b2 = x2[0] * t[0] + x2[1] * t[1] + x2[2] * t[2];
    l1 = b1 - a * b2;
    l2 = -a * b1 + b2;
}

// one record against the four candidates: v[c] += 1 where check_cheirality(candidate c, b1, b2, 0) holds
MDRP_HD void focal_pose_votes(const FocalPoseFrame &fr, const double x1[2], const double x2[2], int v[4]) {
    double b1[3] = {(x1[0] - fr.pp1[0]) / fr.f1, (x1[1] - fr.pp1[1]) / fr.f1, 1.0};
    double b2[3] = {(x2[0] - fr.pp2[0]) / fr.f2, (x2[1] - fr.pp2[1]) / fr.f2, 1.0};
    const double n1 = 1.0 / sqrt(dot3(b1, b1)), n2 = 1.0 / sqrt(dot3(b2, b2));
    for (int k = 0; k < 3; ++k) { b1[k] *= n1; b2[k] *= n2; }
    double l1, l2;
    focal_cheirality_depths(fr.R1, fr.t, b1, b2, l1, l2);   // (R1, t) and (R1, -t)
    v[0] += (l1 > 0.0 && l2 > 0.0) ? 1 : 0;
    v[1] += (-l1 > 0.0 && -l2 > 0.0) ? 1 : 0;
    focal_cheirality_depths(fr.R2, fr.t, b1, b2, l1, l2);   // (R2, t) and (R2, -t)
    v[3] += (l1 > 0.0 && l2 > 0.0) ? 1 : 0;
    v[2] += (-l1 > 0.0 && -l2 > 0.0) ? 1 : 0;
}

// the record from the closed-form part and the votes (votes and voters are not read when the status says that nothing was swept)
MDRP_HD void focal_pose_record(const FocalPoseHead &hd, const int votes[4], int voters, FocalPose &out) {
    model_identity(out.model);
    out.model.f1 = hd.f1; out.model.f2 = hd.f2;
    out.pad_ = 0;
    if (hd.status) {
        for (int c = 0; c < 4; ++c) out.votes[c] = 0;
        out.voters = 0; out.winner = -1; out.status = hd.status;
        return;
    }
    int w = 0;
    for (int c = 1; c < 4; ++c)
        if (votes[c] > votes[w]) w = c; // the largest count, the first one on ties
    for (int c = 0; c < 4; ++c) out.votes[c] = votes[c];
    out.voters = voters; out.winner = w; out.status = voters == 0 ? FOCAL_NO_VOTERS : 0;
    // (the winner without a runtime index into the candidates: they live in LDS on the device, but the host build shares the code)
    const Model &m = w == 0 ? hd.cand[0] : (w == 1 ? hd.cand[1] : (w == 2 ? hd.cand[2] : hd.cand[3]));
    for (int k = 0; k < 4; ++k) out.model.q[k] = m.q[k];
    for (int k = 0; k < 3; ++k) out.model.t[k] = m.t[k];
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------- kernels
// F [count][9] row-major, pp1 / pp2 [count][2] or null (the origin), f1f2 [count][2]
__global__ __launch_bounds__(256) void kc_focals(const double *__restrict__ F, const double *__restrict__ pp1, const double *__restrict__ pp2, int count,
                                                 double *__restrict__ f1f2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double f[9], a[2] = {0.0, 0.0}, b[2] = {0.0, 0.0}, f1, f2;
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = F[(size_t)9 * i + k];
    if (pp1) { a[0] = pp1[2 * (size_t)i]; a[1] = pp1[2 * (size_t)i + 1]; }
    if (pp2) { b[0] = pp2[2 * (size_t)i]; b[1] = pp2[2 * (size_t)i + 1]; }
    focals_from_F(f, a, b, f1, f2);
    f1f2[2 * (size_t)i] = f1; f1f2[2 * (size_t)i + 1] = f2;
}

// x1, x2 [batch][n_max][2]: the caller's pixels; nper [batch]; models: the pair's F row-major in the first nine doubles of the record at
// models + pair * stride (96: packed mdrp_model, 136: mdrp_result); mask [batch][n_max] bytes or null (every record votes); pp1 / pp2 [batch][2] or
// null (the origin).  Rows at or past nper[pair] are not read.  T is fixed, so a pair's record does not depend on its batch.
__global__ __launch_bounds__(FOCAL_POSE_THREADS) void kc_focal_pose(const double *__restrict__ x1, const double *__restrict__ x2, int n_max,
                                                                    const int32_t *__restrict__ nper, const unsigned char *__restrict__ models, int stride,
                                                                    const uint8_t *__restrict__ mask, const double *__restrict__ pp1,
                                                                    const double *__restrict__ pp2, FocalPose *__restrict__ out) {
    constexpr int T = FOCAL_POSE_THREADS, W = T / 64;
    __shared__ FocalPoseHead hd;
    __shared__ int32_t part[W][5];
    const int pair = blockIdx.x;
    const int n = min(max(nper[pair], 0), n_max);
    double a[2] = {0.0, 0.0}, b[2] = {0.0, 0.0};
    if (pp1) { a[0] = pp1[2 * (size_t)pair]; a[1] = pp1[2 * (size_t)pair + 1]; }
    if (pp2) { b[0] = pp2[2 * (size_t)pair]; b[1] = pp2[2 * (size_t)pair + 1]; }
    if (threadIdx.x == 0) { // the closed-form part, once per workgroup
        const double *Fg = reinterpret_cast<const double *>(models + (size_t)pair * stride);
        double F[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] = Fg[k];
        focal_pose_head(F, n, a, b, hd);
    }
    __syncthreads();
    int v[5] = {0, 0, 0, 0, 0}; // four vote counters and the voters
    if (hd.status == 0) {       // (uniform: read from LDS)
        FocalPoseFrame fr;
        focal_pose_frame(hd, a, b, fr);
        const double *p1 = x1 + (size_t)pair * n_max * 2, *p2 = x2 + (size_t)pair * n_max * 2;
        const uint8_t *mk = mask ? mask + (size_t)pair * n_max : nullptr;
        for (int i = threadIdx.x; i < n; i += T) {
            if (mk && mk[i] == 0) continue;
            const double r1[2] = {p1[2 * (size_t)i], p1[2 * (size_t)i + 1]}, r2[2] = {p2[2 * (size_t)i], p2[2 * (size_t)i + 1]};
            focal_pose_votes(fr, r1, r2, v);
            ++v[4];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k)
            for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) part[threadIdx.x >> 6][k] = v[k];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot[5] = {0, 0, 0, 0, 0};
        if (hd.status == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k)
                for (int w = 0; w < W; ++w) tot[k] += part[w][k];
        }
        FocalPose rec;
        focal_pose_record(hd, tot, tot[4], rec);
        out[pair] = rec;
    }
}
#endif

} // namespace mdrp
