// classic_prosac_shim — what tests/tools/gen_golden_classic_prosac.py needs from the REFERENCE's compiled PoseLib:
//   (1) estimate_relative_pose / estimate_shared_focal_relative_pose / estimate_fundamental with RansacOptions::progressive_sampling /
//       max_prosac_iterations set, and
//   (2) RandomSampler::initialize_prosac / generate_sample called directly on an ABI-compatible plain struct with sample_sz = 5, 6, 7.
// Our own code, in the manner of oracle/refshim/refshim.cpp and tests/tools/prosac_shim.cpp: plain structs with the binary's layouts (SURVEY.md
// Appendix A), entry points by mangled name.  TEST INFRASTRUCTURE of the build container only; the generator builds it into oracle/_ref/ (git-ignored).
#include <dlfcn.h>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct alignas(16) V2 { double v[2]; };
struct M33 { double m[9]; };
struct alignas(32) CameraPose { double q[4]; double t[3]; };
struct Camera { int model_id, width, height; std::vector<double> params; };
struct alignas(32) ImagePair { CameraPose pose; Camera camera1, camera2; };
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
struct RandomSampler {
    size_t num_data, sample_sz;
    unsigned long state;
    bool use_prosac;
    size_t max_prosac_iterations, sample_k, subset_sz;
    std::vector<size_t> growth;
};
static_assert(sizeof(RandomSampler) == 80, "RandomSampler layout");

typedef std::vector<V2> VV2;
typedef RansacStats (*est_pose_t)(const VV2 &, const VV2 &, const Camera &, const Camera &, const RansacOptions &, const BundleOptions &, CameraPose *,
                                  std::vector<char> *);
typedef RansacStats (*est_F_t)(const VV2 &, const VV2 &, const RansacOptions &, const BundleOptions &, M33 *, std::vector<char> *);
typedef RansacStats (*est_ip_t)(const VV2 &, const VV2 &, const V2 &, const RansacOptions &, const BundleOptions &, ImagePair *, std::vector<char> *);
typedef void (*init_prosac_t)(RandomSampler *);
typedef void (*gen_sample_t)(RandomSampler *, std::vector<size_t> *);

void *H = nullptr;
est_pose_t f_est_relpose;
est_F_t f_est_F;
est_ip_t f_est_sf;
init_prosac_t f_init_prosac;
gen_sample_t f_gen_sample;

template <typename T> bool sym(T &f, const char *name) {
    f = (T)dlsym(H, name);
    if (!f) fprintf(stderr, "classic_prosac_shim: missing symbol %s\n", name);
    return f != nullptr;
}
VV2 mk2(const double *x, int n) {
    VV2 v(n);
    for (int i = 0; i < n; ++i) { v[i].v[0] = x[2 * i]; v[i].v[1] = x[2 * i + 1]; }
    return v;
}
RandomSampler sampler(size_t n, size_t ssz, unsigned long seed, size_t max_prosac_iterations) {
    RandomSampler rs;
    rs.num_data = n; rs.sample_sz = ssz; rs.state = seed; rs.use_prosac = true; rs.max_prosac_iterations = max_prosac_iterations;
    rs.sample_k = 0; rs.subset_sz = 0;
    f_init_prosac(&rs);
    return rs;
}

} // namespace

extern "C" {

int cshim_init(const char *so_path) {
    if (H) return 0;
    H = dlopen(so_path, RTLD_LAZY | RTLD_GLOBAL);
    if (!H) { fprintf(stderr, "classic_prosac_shim: dlopen failed: %s\n", dlerror()); return -1; }
    bool ok = true;
    ok &= sym(f_est_relpose, "_ZN7poselib22estimate_relative_poseERKSt6vectorIN5Eigen6MatrixIdLi2ELi1ELi0ELi2ELi1EEESaIS3_EES7_RKNS_6CameraESA_RKNS_13RansacOptionsERKNS_13BundleOptionsEPNS_10CameraPoseEPS0_IcSaIcEE");
    ok &= sym(f_est_F, "_ZN7poselib20estimate_fundamentalERKSt6vectorIN5Eigen6MatrixIdLi2ELi1ELi0ELi2ELi1EEESaIS3_EES7_RKNS_13RansacOptionsERKNS_13BundleOptionsEPNS2_IdLi3ELi3ELi0ELi3ELi3EEEPS0_IcSaIcEE");
    ok &= sym(f_est_sf, "_ZN7poselib35estimate_shared_focal_relative_poseERKSt6vectorIN5Eigen6MatrixIdLi2ELi1ELi0ELi2ELi1EEESaIS3_EES7_RKS3_RKNS_13RansacOptionsERKNS_13BundleOptionsEPNS_9ImagePairEPS0_IcSaIcEE");
    ok &= sym(f_init_prosac, "_ZN7poselib13RandomSampler17initialize_prosacEv");
    ok &= sym(f_gen_sample, "_ZN7poselib13RandomSampler15generate_sampleEPSt6vectorImSaImEE");
    return ok ? 0 : -2;
}

// growth: max(n, ssz) entries; samples: [count][ssz]; subset: the sampler's subset_sz before each draw, [count]
void cshim_sampler(size_t n, size_t ssz, unsigned long seed, size_t max_prosac_iterations, int count, long long *growth, long long *samples, long long *subset) {
    RandomSampler rs = sampler(n, ssz, seed, max_prosac_iterations);
    for (size_t i = 0; i < rs.growth.size(); ++i) growth[i] = (long long)rs.growth[i];
    std::vector<size_t> s(ssz);
    for (int i = 0; i < count; ++i) {
        subset[i] = (long long)rs.subset_sz;
        f_gen_sample(&rs, &s);
        for (size_t k = 0; k < ssz; ++k) samples[ssz * i + k] = (long long)s[k];
    }
}
int cshim_growth_len(size_t n, size_t ssz, size_t max_prosac_iterations) { return (int)sampler(n, ssz, 0, max_prosac_iterations).growth.size(); }

// kind 3 relative pose (cam: model_id, width, height, nparams, params...; model out: q t), 4 shared focal (pp[2]; model out: q t f), 5 fundamental
// (model out: nine entries, column-major).  ropt9: max_it, min_it, dyn_mult, success_prob, max_reproj, max_epi, seed, progressive_sampling,
// max_prosac_iterations.  bopt8: max_it, loss_type, loss_scale, grad_tol, step_tol, lambda0, min_lambda, max_lambda.
void cshim_estimate(int kind, const double *x1, const double *x2, int n, const double *cam1, const double *cam2, const double *pp, const double *o,
                    const double *bo, double *model9, double *stats5, unsigned char *mask) {
    RansacOptions r;
    memset(&r, 0, sizeof r);
    r.max_iterations = (size_t)o[0]; r.min_iterations = (size_t)o[1];
    r.dyn_num_trials_mult = o[2]; r.success_prob = o[3]; r.max_reproj_error = o[4]; r.max_epipolar_error = o[5];
    r.seed = (unsigned long)o[6]; r.progressive_sampling = o[7] != 0.0; r.max_prosac_iterations = (size_t)o[8];
    r.monodepth_weight_sampson = 1.0f;
    BundleOptions b;
    memset(&b, 0, sizeof b);
    b.max_iterations = (size_t)bo[0]; b.loss_type = (int)bo[1]; b.loss_scale = bo[2]; b.gradient_tol = bo[3];
    b.step_tol = bo[4]; b.initial_lambda = bo[5]; b.min_lambda = bo[6]; b.max_lambda = bo[7];
    std::vector<char> inl;
    RansacStats s;
    const VV2 a1 = mk2(x1, n), a2 = mk2(x2, n);
    memset(model9, 0, 9 * sizeof(double));
    srand(1); // the binary's solvers call rand(): one fixed state per call
    if (kind == 3) {
        Camera c1, c2;
        c1.model_id = (int)cam1[0]; c1.width = (int)cam1[1]; c1.height = (int)cam1[2]; c1.params.assign(cam1 + 4, cam1 + 4 + (int)cam1[3]);
        c2.model_id = (int)cam2[0]; c2.width = (int)cam2[1]; c2.height = (int)cam2[2]; c2.params.assign(cam2 + 4, cam2 + 4 + (int)cam2[3]);
        CameraPose p;
        memset(&p, 0, sizeof p); p.q[0] = 1.0;
        s = f_est_relpose(a1, a2, c1, c2, r, b, &p, &inl);
        memcpy(model9, p.q, 32); memcpy(model9 + 4, p.t, 24);
    } else if (kind == 4) {
        ImagePair ip;
        memset(&ip.pose, 0, sizeof ip.pose); ip.pose.q[0] = 1.0;
        ip.camera1.model_id = 0; ip.camera1.width = 0; ip.camera1.height = 0; ip.camera1.params = {1.0, 0.0, 0.0};
        ip.camera2 = ip.camera1;
        V2 c; c.v[0] = pp[0]; c.v[1] = pp[1];
        s = f_est_sf(a1, a2, c, r, b, &ip, &inl);
        memcpy(model9, ip.pose.q, 32); memcpy(model9 + 4, ip.pose.t, 24);
        model9[7] = ip.camera1.params.empty() ? 0.0 : ip.camera1.params[0];
    } else {
        M33 F;
        memset(&F, 0, sizeof F); F.m[0] = F.m[4] = F.m[8] = 1.0;
        s = f_est_F(a1, a2, r, b, &F, &inl);
        memcpy(model9, F.m, 72);
    }
    stats5[0] = (double)s.refinements; stats5[1] = (double)s.iterations; stats5[2] = (double)s.num_inliers; stats5[3] = s.inlier_ratio; stats5[4] = s.model_score;
    for (int i = 0; i < n; ++i) mask[i] = (i < (int)inl.size()) ? (unsigned char)(inl[i] != 0) : 0;
}

} // extern "C"
