// Host build of the varying-focal baseline's tail (mdrp_amd/csrc/mdrp_classic_focals.h: focals_from_F, focal_pose_head, focal_pose_votes,
// focal_pose_record — what kc_focals and kc_focal_pose apply) for tests/test_classic_focals_host.py: a pair's records walked in order on the CPU,
// plain C entry points over arrays, no GPU.
//   g++ -O2 -std=c++17 -fPIC -shared focals_host.cpp -o libfocals_host.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DFOCALS_HOST_MAIN focals_host.cpp -o focals_host_san   (stand-alone)
#include "../../mdrp_amd/csrc/mdrp_classic_focals.h"

#include <cstddef>
#include <cstdio>
#include <vector>

using namespace mdrp;

extern "C" {

int fh_record_bytes() { return (int)sizeof(FocalPose); }
// offsets of votes, voters, winner, status, pad_
void fh_record_offsets(int *o) {
    o[0] = (int)offsetof(FocalPose, votes); o[1] = (int)offsetof(FocalPose, voters); o[2] = (int)offsetof(FocalPose, winner);
    o[3] = (int)offsetof(FocalPose, status); o[4] = (int)offsetof(FocalPose, pad_);
}

// F [count][9] row-major; pp1, pp2 [count][2] or null; f1f2 [count][2]
void fh_focals(const double *F, const double *pp1, const double *pp2, int count, double *f1f2) {
    const double zero[2] = {0.0, 0.0};
    for (int i = 0; i < count; ++i)
        focals_from_F(F + 9 * (size_t)i, pp1 ? pp1 + 2 * (size_t)i : zero, pp2 ? pp2 + 2 * (size_t)i : zero, f1f2[2 * (size_t)i], f1f2[2 * (size_t)i + 1]);
}

// one pair as kc_focal_pose treats it: x1, x2 [n_max][2] of which the first n are read, mask [n_max] or null.  out: the 128-byte record;
// cand [4][12]: the four candidates (identity where the status says that there are none)
void fh_pose(const double *x1, const double *x2, int n_max, int n, const double *F, const unsigned char *mask, const double *pp1, const double *pp2,
             void *out, double *cand) {
    const double zero[2] = {0.0, 0.0};
    const double *a = pp1 ? pp1 : zero, *b = pp2 ? pp2 : zero;
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    FocalPoseHead hd;
    focal_pose_head(F, n, a, b, hd);
    int v[4] = {0, 0, 0, 0}, voters = 0;
    if (hd.status == 0) {
        FocalPoseFrame fr;
        focal_pose_frame(hd, a, b, fr);
        for (int i = 0; i < n; ++i) {
            if (mask && mask[i] == 0) continue;
            focal_pose_votes(fr, x1 + 2 * (size_t)i, x2 + 2 * (size_t)i, v);
            ++voters;
        }
    }
    focal_pose_record(hd, v, voters, *static_cast<FocalPose *>(out));
    for (int c = 0; c < 4; ++c) {
        const double *m = reinterpret_cast<const double *>(&hd.cand[c]);
        for (int k = 0; k < 12; ++k) cand[12 * c + k] = m[k];
    }
}

} // extern "C"

#ifdef FOCALS_HOST_MAIN
// stand-alone run for the sanitizers: a synthetic pair (two pinhole cameras, points in front of both), rows past n poisoned with NaN
int main() {
    const int n_max = 70, n = 65;
    const double f1 = 900.0, f2 = 1100.0, pp1[2] = {12.0, -7.0}, pp2[2] = {-5.0, 9.0};
    const double c = 0.9950041652780258, s = 0.09983341664682815; // a rotation of 0.1 rad about y
    const double R[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, t[3] = {0.8, 0.1, 0.2};
    std::vector<double> x1(2 * n_max, NAN), x2(2 * n_max, NAN);
    std::vector<unsigned char> mask(n_max, 1);
    for (int i = 0; i < n; ++i) {
        const double X[3] = {-1.0 + 0.031 * i, 0.7 - 0.023 * i, 4.0 + 0.05 * (i % 11)};
        const double Y[3] = {R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1], R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]};
        x1[2 * i] = f1 * X[0] / X[2] + pp1[0]; x1[2 * i + 1] = f1 * X[1] / X[2] + pp1[1];
        x2[2 * i] = f2 * Y[0] / Y[2] + pp2[0]; x2[2 * i + 1] = f2 * Y[1] / Y[2] + pp2[1];
        mask[i] = i % 5 != 0;
    }
    // F = K2^-T [t]x R K1^-1
    const double tx[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
    double E[9], F[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) E[3 * i + j] = tx[3 * i] * R[j] + tx[3 * i + 1] * R[3 + j] + tx[3 * i + 2] * R[6 + j];
    const double K1i[9] = {1 / f1, 0, -pp1[0] / f1, 0, 1 / f1, -pp1[1] / f1, 0, 0, 1}, K2i[9] = {1 / f2, 0, -pp2[0] / f2, 0, 1 / f2, -pp2[1] / f2, 0, 0, 1};
    double M[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[3 * i + j] = E[3 * i] * K1i[j] + E[3 * i + 1] * K1i[3 + j] + E[3 * i + 2] * K1i[6 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) F[3 * i + j] = K2i[i] * M[j] + K2i[3 + i] * M[3 + j] + K2i[6 + i] * M[6 + j];
    FocalPose rec;
    double cand[48];
    fh_pose(x1.data(), x2.data(), n_max, n, F, mask.data(), pp1, pp2, &rec, cand);
    const bool ok = rec.status == 0 && rec.voters == 52 && rec.votes[rec.winner] == 52 && fabs(rec.model.f1 - f1) < 1e-6 * f1 && fabs(rec.model.f2 - f2) < 1e-6 * f2;
    double ff[2];
    fh_focals(F, pp1, pp2, 1, ff);
    F[0] = NAN;
    fh_pose(x1.data(), x2.data(), n_max, n, F, nullptr, nullptr, nullptr, &rec, cand);
    if (!ok || rec.status != FOCAL_NO_MODEL || rec.winner != -1 || ff[0] != ff[0]) { printf("focals_host: FAILED\n"); return 1; }
    printf("focals_host: ok\n");
    return 0;
}
#endif
