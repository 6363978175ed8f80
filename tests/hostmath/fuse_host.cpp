// Host build of the consistency filter's arithmetic (mdrp_amd/csrc/mdrp_fuse.h: a view's record, F3's slots, and fuse_decide, the one function
// through which both kernels decide) for tests/test_fuse_host.py, which pins it against the NumPy definition without a GPU.  Plain C++: g++ fuses
// nothing on x86-64 without -mfma, which is the rounding the kernels are held to by recon_mul.  A stand-alone program:
//     fuse_host <in> <out>
// in:  uint32 hdr[12] = kind, I, H, W, V, keep, min_consistent, max_violating, thr, seed, 0, 0 | double lo, hi | I transform records (128 bytes each) |
//      I cameras (40 bytes each; zeros for a focal kind) | I centres (2 doubles) | I sizes (2 int32) | I * V views (int32) | I * H * W depths (double)
// out: per image and pixel of the allocation 3 bytes: n_cons, n_viol, flags (bit 0: a candidate, bit 1: kept); 0, 0, 0 outside the valid region
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../mdrp_amd/csrc/mdrp_fuse.h"

using namespace mdrp;

template <typename T>
static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: fuse_host <in> <out>\n"); return 2; }
    static_assert(sizeof(SceneTransform) == 128 && sizeof(ReconCam) == 40 && sizeof(FuseView) == 184 && sizeof(FuseRow) == 36, "layouts");
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<uint32_t> hdr = take<uint32_t>(f, 12);
    const int kind = (int)hdr[0], I = (int)hdr[1], H = (int)hdr[2], W = (int)hdr[3], V = (int)hdr[4], keep = (int)hdr[5];
    const std::vector<double> band = take<double>(f, 2);
    const FuseGate gate{band[0], band[1], (int32_t)hdr[6], (int32_t)hdr[7]};
    const uint32_t thr = hdr[8], seed = hdr[9];
    const std::vector<SceneTransform> T = take<SceneTransform>(f, (size_t)I);
    const std::vector<ReconCam> cams = take<ReconCam>(f, (size_t)I);
    const std::vector<double> centre = take<double>(f, 2 * (size_t)I);
    const std::vector<int32_t> size = take<int32_t>(f, 2 * (size_t)I);
    const std::vector<int32_t> views = take<int32_t>(f, (size_t)I * (size_t)V);
    const std::vector<double> depth = take<double>(f, (size_t)I * (size_t)H * (size_t)W);
    fclose(f);

    std::vector<FuseView> fv((size_t)I);
    std::vector<FuseRow> fr((size_t)I);
    std::vector<SceneImage> im((size_t)I);
    for (int i = 0; i < I; ++i) {
        const bool attached = T[i].depth >= 0;
        const int h = attached ? fe_clamp_extent(size[2 * i], H) : 0, w = attached ? fe_clamp_extent(size[2 * i + 1], W) : 0;
        const ReconCam *cam = kind == 0 ? &cams[i] : nullptr;
        fv[i] = fuse_view(T[i], kind, cam, centre[2 * i], centre[2 * i + 1], h, w, (size_t)i * (size_t)H * (size_t)W);
        fuse_slots(T.data(), I, i, views.data() + (size_t)i * (size_t)V, V, fr[i]);
        im[i] = scene_image(T[i], kind, cam);
    }
    const double *map = depth.data();
    const size_t stride = (size_t)W;
    const auto ld = [map, stride](const FuseView &g, uint32_t vt, uint32_t ut) { return map[g.base + (size_t)vt * stride + (size_t)ut]; };
    std::vector<unsigned char> out((size_t)I * (size_t)H * (size_t)W * 3, 0);
    for (int i = 0; i < I; ++i)
        for (int v = 0; v < fv[i].h; ++v)
            for (int u = 0; u < fv[i].w; ++u) {
                const size_t at = fv[i].base + (size_t)v * stride + (size_t)u;
                if (!recon_candidate(thr, scene_seed(seed, (uint32_t)i), SCENE_STAGE, (uint32_t)v, (uint32_t)u)) continue;
                const double d[1] = {map[at]};
                if (!recon_keep(d[0], keep)) continue;
                double Q[1][3];
                scene_point(T[i], im[i], (uint32_t)v, (uint32_t)u, fv[i].c0, fv[i].c1, d[0], Q[0]);
                unsigned support[1];
                const unsigned kept = fuse_decide<1>(1u, d, T[i].shift, Q, fr[i], fv.data(), gate, ld, support);
                out[3 * at] = (unsigned char)(support[0] & 0xFFu); out[3 * at + 1] = (unsigned char)(support[0] >> 8);
                out[3 * at + 2] = (unsigned char)(1u | (kept << 1));
            }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { perror(argv[2]); return 2; }
    fclose(f);
    return 0;
}
