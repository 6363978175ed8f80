// classic_focals_shim — what tests/tools/gen_golden_classic_focals.py needs from the REFERENCE's compiled PoseLib: focals_from_fundamental(F, pp1, pp2).
// Our own code, in the manner of tests/tools/classic_initial_F_shim.cpp: plain structs with the binary's layouts, the entry point
// by its mangled name.  TEST INFRASTRUCTURE of the build container only; the generator builds it into oracle/_ref/ (git-ignored).
#include <dlfcn.h>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

namespace {

struct alignas(16) V2 { double v[2]; };
struct M33 { double m[9]; }; // column-major, as the binary holds it
struct Camera { int model_id, width, height; std::vector<double> params; };
typedef std::pair<Camera, Camera> (*focals_t)(const M33 &, const V2 &, const V2 &);

void *H = nullptr;
focals_t f_focals;

} // namespace

extern "C" {

int focshim_init(const char *so_path) {
    if (H) return 0;
    H = dlopen(so_path, RTLD_LAZY | RTLD_GLOBAL);
    if (!H) { fprintf(stderr, "classic_focals_shim: dlopen failed: %s\n", dlerror()); return -1; }
    f_focals = (focals_t)dlsym(H, "_ZN7poselib23focals_from_fundamentalERKN5Eigen6MatrixIdLi3ELi3ELi0ELi3ELi3EEERKNS1_IdLi2ELi1ELi0ELi2ELi1EEES7_");
    if (!f_focals) { fprintf(stderr, "classic_focals_shim: missing symbol focals_from_fundamental\n"); return -2; }
    return 0;
}

// F: [count][9] ROW-major; pp1, pp2: [count][2].  cams: [count][2][6] = model_id, width, height, and the three parameters of each returned camera
// (NaN where it has fewer).  Returns the number of cameras that did not come back with three parameters.
int focshim_focals(const double *F, const double *pp1, const double *pp2, int count, double *cams) {
    int odd = 0;
    for (int i = 0; i < count; ++i) {
        M33 Fc;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Fc.m[3 * c + r] = F[9 * i + 3 * r + c];
        V2 a, b;
        a.v[0] = pp1[2 * i]; a.v[1] = pp1[2 * i + 1];
        b.v[0] = pp2[2 * i]; b.v[1] = pp2[2 * i + 1];
        const std::pair<Camera, Camera> pc = f_focals(Fc, a, b);
        const Camera *cs[2] = {&pc.first, &pc.second};
        for (int k = 0; k < 2; ++k) {
            double *o = cams + 12 * i + 6 * k;
            o[0] = cs[k]->model_id; o[1] = cs[k]->width; o[2] = cs[k]->height;
            if (cs[k]->params.size() != 3) ++odd;
            for (size_t j = 0; j < 3; ++j) o[3 + j] = j < cs[k]->params.size() ? cs[k]->params[j] : __builtin_nan("");
        }
    }
    return odd;
}

} // extern "C"
