// Host build of the scene header's arithmetic (mdrp_amd/csrc/mdrp_scene.h: the per-image seed, the tree's edges, the accumulation along the tree, the
// image's record and the point of a kept pixel) for tests/test_scene_host.py, which pins it against the NumPy definition without a GPU.  Plain C++:
// g++ fuses nothing on x86-64 without -mfma, which is the rounding the kernels are held to by recon_mul.
#include "../../mdrp_amd/csrc/mdrp_scene.h"

using namespace mdrp;

extern "C" {

void sh_limits(int *out) {
    out[0] = SCENE_ABSENT; out[1] = SCENE_EDGE; out[2] = SCENE_ROOT; out[3] = (int)SCENE_STAGE; out[4] = (int)sizeof(SceneTransform); out[5] = (int)sizeof(SceneImage);
}

uint32_t sh_seed(uint32_t seed, uint32_t image) { return scene_seed(seed, image); }

// S1 and S2: the records of all n_images images
void sh_transforms(int kind, int batch, const void *models, int stride, const int32_t *pairs, int n_images, const int32_t *tree, SceneTransform *out) {
    const SceneTree s{static_cast<const unsigned char *>(models), pairs, tree, stride, kind, batch, n_images};
    for (int i = 0; i < n_images; ++i) scene_chain(s, i, out[i]);
}

// S5 and S6: n pixels (v, u) with depths d of an image with record T and camera (id, params; null for a focal kind): out[n][3] float, the rounded points
void sh_points(const SceneTransform *T, int kind, int cam_id, const double *cam_params, double c0, double c1, int n, const uint32_t *v, const uint32_t *u,
               const double *d, float *out) {
    ReconCam cam{};
    cam.model_id = cam_id;
    for (int k = 0; k < 4; ++k) cam.params[k] = cam_params ? cam_params[k] : 0.0;
    const SceneImage im = scene_image(*T, kind, cam_params ? &cam : nullptr);
    for (int i = 0; i < n; ++i) {
        double o[3];
        scene_point(*T, im, v[i], u[i], c0, c1, d[i], o);
        out[3 * i] = (float)o[0]; out[3 * i + 1] = (float)o[1]; out[3 * i + 2] = (float)o[2];
    }
}

}
