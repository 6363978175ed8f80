// prosac_shim — what tests/tools/gen_golden_prosac.py needs from the REFERENCE's compiled PoseLib beyond oracle/refshim/refshim.cpp:
//   (1) the three monodepth estimators with RansacOptions::progressive_sampling / max_prosac_iterations set, and
//   (2) RandomSampler::initialize_prosac / generate_sample called directly on an ABI-compatible plain struct.
// Our own code, in the manner of refshim.cpp: plain structs with the binary's layouts, entry points by mangled name.
// TEST INFRASTRUCTURE of the build container only; the generator builds it into oracle/_ref/ (git-ignored).
#include <dlfcn.h>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct alignas(16) V2 { double v[2]; };
struct alignas(32) CameraPose { double q[4]; double t[3]; };
struct alignas(32) MDG { CameraPose pose; double scale, shift1, shift2; };
struct Camera { int model_id, width, height; std::vector<double> params; };
struct alignas(32) MDIP { MDG geometry; Camera camera1, camera2; };
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
// RandomSampler (@0x38 .. 0x88 of the estimator objects)
struct RandomSampler {
    size_t num_data, sample_sz;
    unsigned long state;
    bool use_prosac;
    size_t max_prosac_iterations, sample_k, subset_sz;
    std::vector<size_t> growth;
};
static_assert(sizeof(RandomSampler) == 80, "RandomSampler layout");

typedef std::vector<V2> VV2;
typedef std::vector<double> VD;
typedef RansacStats (*est_calib_t)(const VV2 &, const VV2 &, const VD &, const VD &, const Camera &, const Camera &, const RansacOptions &,
                                   const BundleOptions &, MDG *, std::vector<char> *);
typedef RansacStats (*est_focal_t)(const VV2 &, const VV2 &, const VD &, const VD &, const RansacOptions &, const BundleOptions &, MDIP *,
                                   std::vector<char> *);
typedef void (*init_prosac_t)(RandomSampler *);
typedef void (*gen_sample_t)(RandomSampler *, std::vector<size_t> *);

void *H = nullptr;
est_calib_t f_est_calib;
est_focal_t f_est_shared, f_est_varying;
init_prosac_t f_init_prosac;
gen_sample_t f_gen_sample;

template <typename T> bool sym(T &f, const char *name) {
    f = (T)dlsym(H, name);
    if (!f) fprintf(stderr, "prosac_shim: missing symbol %s\n", name);
    return f != nullptr;
}
VV2 mk2(const double *x, int n) {
    VV2 v(n);
    for (int i = 0; i < n; ++i) { v[i].v[0] = x[2 * i]; v[i].v[1] = x[2 * i + 1]; }
    return v;
}

} // namespace

extern "C" {

int pshim_init(const char *so_path) {
    if (H) return 0;
    H = dlopen(so_path, RTLD_LAZY | RTLD_GLOBAL);
    if (!H) { fprintf(stderr, "prosac_shim: dlopen failed: %s\n", dlerror()); return -1; }
    bool ok = true;
    ok &= sym(f_est_calib, "_ZN7poselib32estimate_monodepth_relative_poseERKSt6vectorIN5Eigen6MatrixIdLi2ELi1ELi0ELi2ELi1EEESaIS3_EES7_RKS0_IdSaIdEESB_RKNS_6CameraESE_RKNS_13RansacOptionsERKNS_13BundleOptionsEPNS_24MonoDepthTwoViewGeometryEPS0_IcSaIcEE");
    ok &= sym(f_est_shared, "_ZN7poselib45estimate_shared_focal_monodepth_relative_poseERKSt6vectorIN5Eigen6MatrixIdLi2ELi1ELi0ELi2ELi1EEESaIS3_EES7_RKS0_IdSaIdEESB_RKNS_13RansacOptionsERKNS_13BundleOptionsEPNS_18MonoDepthImagePairEPS0_IcSaIcEE");
    ok &= sym(f_est_varying, "_ZN7poselib46estimate_varying_focal_monodepth_relative_poseERKSt6vectorIN5Eigen6MatrixIdLi2ELi1ELi0ELi2ELi1EEESaIS3_EES7_RKS0_IdSaIdEESB_RKNS_13RansacOptionsERKNS_13BundleOptionsEPNS_18MonoDepthImagePairEPS0_IcSaIcEE");
    ok &= sym(f_init_prosac, "_ZN7poselib13RandomSampler17initialize_prosacEv");
    ok &= sym(f_gen_sample, "_ZN7poselib13RandomSampler15generate_sampleEPSt6vectorImSaImEE");
    return ok ? 0 : -2;
}

// growth: max(n, 3) entries; samples: [count][3]; subset: the sampler's subset_sz before each draw, [count]
void pshim_sampler(size_t n, unsigned long seed, size_t max_prosac_iterations, int count, long long *growth, long long *samples, long long *subset) {
    RandomSampler rs;
    rs.num_data = n; rs.sample_sz = 3; rs.state = seed; rs.use_prosac = true; rs.max_prosac_iterations = max_prosac_iterations;
    rs.sample_k = 0; rs.subset_sz = 0;
    f_init_prosac(&rs);
    for (size_t i = 0; i < rs.growth.size(); ++i) growth[i] = (long long)rs.growth[i];
    std::vector<size_t> s(3);
    for (int i = 0; i < count; ++i) {
        subset[i] = (long long)rs.subset_sz;
        f_gen_sample(&rs, &s);
        for (int k = 0; k < 3; ++k) samples[3 * i + k] = (long long)s[k];
    }
}
int pshim_growth_len(size_t n, size_t max_prosac_iterations) {
    RandomSampler rs;
    rs.num_data = n; rs.sample_sz = 3; rs.state = 0; rs.use_prosac = true; rs.max_prosac_iterations = max_prosac_iterations;
    rs.sample_k = 0; rs.subset_sz = 0;
    f_init_prosac(&rs);
    return (int)rs.growth.size();
}

// kind 0 calibrated (cam: model_id, width, height, nparams, params...), 1 shared, 2 varying focal.
// ropt11: max_it, min_it, dyn_mult, success_prob, max_reproj, max_epi, seed, estimate_shift, weight_sampson, progressive_sampling, max_prosac_iterations
// bopt8: max_it, loss_type, loss_scale, grad_tol, step_tol, lambda0, min_lambda, max_lambda.  model: q t scale shift1 shift2 f1 f2 (12), out.
void pshim_estimate(int kind, const double *x1, const double *x2, const double *d1, const double *d2, int n, const double *cam1, const double *cam2,
                    const double *o, const double *bo, double *model, double *stats5, unsigned char *mask) {
    RansacOptions r;
    memset(&r, 0, sizeof r);
    r.max_iterations = (size_t)o[0]; r.min_iterations = (size_t)o[1];
    r.dyn_num_trials_mult = o[2]; r.success_prob = o[3]; r.max_reproj_error = o[4]; r.max_epipolar_error = o[5];
    r.seed = (unsigned long)o[6]; r.monodepth_estimate_shift = o[7] != 0.0; r.monodepth_weight_sampson = (float)o[8];
    r.progressive_sampling = o[9] != 0.0; r.max_prosac_iterations = (size_t)o[10];
    BundleOptions b;
    memset(&b, 0, sizeof b);
    b.max_iterations = (size_t)bo[0]; b.loss_type = (int)bo[1]; b.loss_scale = bo[2]; b.gradient_tol = bo[3];
    b.step_tol = bo[4]; b.initial_lambda = bo[5]; b.min_lambda = bo[6]; b.max_lambda = bo[7];
    std::vector<char> inl;
    RansacStats s;
    MDIP p;
    memset(p.geometry.pose.q, 0, sizeof p.geometry.pose.q); memset(p.geometry.pose.t, 0, sizeof p.geometry.pose.t);
    p.geometry.pose.q[0] = 1.0; p.geometry.scale = 1.0; p.geometry.shift1 = 0.0; p.geometry.shift2 = 0.0;
    p.camera1.model_id = 0; p.camera1.width = 0; p.camera1.height = 0; p.camera1.params = {1.0, 0.0, 0.0};
    p.camera2 = p.camera1;
    const VV2 a1 = mk2(x1, n), a2 = mk2(x2, n);
    const VD e1(d1, d1 + n), e2(d2, d2 + n);
    srand(1); // the binary's solvers call rand() (see tests/tools: the headline reference generator): one fixed state per call
    if (kind == 0) {
        Camera c1, c2;
        c1.model_id = (int)cam1[0]; c1.width = (int)cam1[1]; c1.height = (int)cam1[2]; c1.params.assign(cam1 + 4, cam1 + 4 + (int)cam1[3]);
        c2.model_id = (int)cam2[0]; c2.width = (int)cam2[1]; c2.height = (int)cam2[2]; c2.params.assign(cam2 + 4, cam2 + 4 + (int)cam2[3]);
        s = f_est_calib(a1, a2, e1, e2, c1, c2, r, b, &p.geometry, &inl);
    } else
        s = (kind == 1 ? f_est_shared : f_est_varying)(a1, a2, e1, e2, r, b, &p, &inl);
    memcpy(model, p.geometry.pose.q, 32); memcpy(model + 4, p.geometry.pose.t, 24);
    model[7] = p.geometry.scale; model[8] = p.geometry.shift1; model[9] = p.geometry.shift2;
    model[10] = kind == 0 || p.camera1.params.empty() ? 1.0 : p.camera1.params[0];
    model[11] = kind == 0 || p.camera2.params.empty() ? 1.0 : p.camera2.params[0];
    stats5[0] = (double)s.refinements; stats5[1] = (double)s.iterations; stats5[2] = (double)s.num_inliers; stats5[3] = s.inlier_ratio; stats5[4] = s.model_score;
    for (int i = 0; i < n; ++i) mask[i] = (i < (int)inl.size()) ? (unsigned char)(inl[i] != 0) : 0;
}

} // extern "C"
