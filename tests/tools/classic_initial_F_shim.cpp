// classic_initial_F_shim — what tests/tools/gen_golden_classic_initial_F.py needs from the REFERENCE's compiled PoseLib: estimate_fundamental called
// with a caller's matrix in *F (the Python wrapper's initial_F) and with RansacOptions::score_initial_model set or not.
// Our own code, in the manner of tests/tools/classic_prosac_shim.cpp: plain structs with the binary's layouts, the entry point
// by its mangled name.  TEST INFRASTRUCTURE of the build container only; the generator builds it into oracle/_ref/ (git-ignored).
#include <dlfcn.h>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct alignas(16) V2 { double v[2]; };
struct M33 { double m[9]; };
struct RansacOptions {
    size_t max_iterations, min_iterations;
    double dyn_num_trials_mult, success_prob, max_reproj_error, max_epipolar_error;
    unsigned long seed;
    bool progressive_sampling;
    size_t max_prosac_iterations;
    bool real_focal_check, score_initial_model, monodepth_estimate_shift;
    float monodepth_weight_sampson;
};
struct BundleOptions {
    size_t max_iterations;
    int loss_type;
    double loss_scale, gradient_tol, step_tol, initial_lambda, min_lambda, max_lambda;
    bool verbose;
};
struct RansacStats { size_t refinements, iterations, num_inliers; double inlier_ratio, model_score; };
typedef std::vector<V2> VV2;
typedef RansacStats (*est_F_t)(const VV2 &, const VV2 &, const RansacOptions &, const BundleOptions &, M33 *, std::vector<char> *);

void *H = nullptr;
est_F_t f_est_F;

VV2 mk2(const double *x, int n) {
    VV2 v(n);
    for (int i = 0; i < n; ++i) { v[i].v[0] = x[2 * i]; v[i].v[1] = x[2 * i + 1]; }
    return v;
}

} // namespace

extern "C" {

int fshim_init(const char *so_path) {
    if (H) return 0;
    H = dlopen(so_path, RTLD_LAZY | RTLD_GLOBAL);
    if (!H) { fprintf(stderr, "classic_initial_F_shim: dlopen failed: %s\n", dlerror()); return -1; }
    f_est_F = (est_F_t)dlsym(H, "_ZN7poselib20estimate_fundamentalERKSt6vectorIN5Eigen6MatrixIdLi2ELi1ELi0ELi2ELi1EEESaIS3_EES7_RKNS_13RansacOptionsERKNS_13BundleOptionsEPNS2_IdLi3ELi3ELi0ELi3ELi3EEEPS0_IcSaIcEE");
    if (!f_est_F) { fprintf(stderr, "classic_initial_F_shim: missing symbol estimate_fundamental\n"); return -2; }
    return 0;
}

// F9: the matrix handed in and returned, column-major as the binary holds it.  ropt8: max_it, min_it, dyn_mult, success_prob, max_reproj, max_epi,
// seed, score_initial_model.  bopt8: max_it, loss_type, loss_scale, grad_tol, step_tol, lambda0, min_lambda, max_lambda.
void fshim_estimate(const double *x1, const double *x2, int n, const double *o, const double *bo, double *F9, double *stats5, unsigned char *mask) {
    RansacOptions r;
    memset(&r, 0, sizeof r);
    r.max_iterations = (size_t)o[0]; r.min_iterations = (size_t)o[1];
    r.dyn_num_trials_mult = o[2]; r.success_prob = o[3]; r.max_reproj_error = o[4]; r.max_epipolar_error = o[5];
    r.seed = (unsigned long)o[6]; r.score_initial_model = o[7] != 0.0;
    r.max_prosac_iterations = 100000;
    r.monodepth_weight_sampson = 1.0f;
    BundleOptions b;
    memset(&b, 0, sizeof b);
    b.max_iterations = (size_t)bo[0]; b.loss_type = (int)bo[1]; b.loss_scale = bo[2]; b.gradient_tol = bo[3];
    b.step_tol = bo[4]; b.initial_lambda = bo[5]; b.min_lambda = bo[6]; b.max_lambda = bo[7];
    std::vector<char> inl;
    const VV2 a1 = mk2(x1, n), a2 = mk2(x2, n);
    M33 F;
    memcpy(F.m, F9, 72);
    srand(1); // the binary's solvers call rand(): one fixed state per call
    const RansacStats s = f_est_F(a1, a2, r, b, &F, &inl);
    memcpy(F9, F.m, 72);
    stats5[0] = (double)s.refinements; stats5[1] = (double)s.iterations; stats5[2] = (double)s.num_inliers; stats5[3] = s.inlier_ratio; stats5[4] = s.model_score;
    for (int i = 0; i < n; ++i) mask[i] = (i < (int)inl.size()) ? (unsigned char)(inl[i] != 0) : 0;
}

} // extern "C"
