// Host build of the per-image rules of the front end (mdrp_amd/csrc/mdrp_frontend.h, k_gather_images) for tests/test_image_pairs_host.py:
// plain C entry points over arrays, no GPU.  g++ -O2 -std=c++17 -fPIC -shared image_pairs_host.cpp -o libimage_pairs_host.so
#include "../../mdrp_amd/csrc/mdrp_frontend.h"

using namespace mdrp;

extern "C" {

void ih_image_valid(const int *a, int count, int n_images, int *ok) {
    for (int k = 0; k < count; ++k) ok[k] = fe_image_valid(a[k], n_images) ? 1 : 0;
}
void ih_clamp_extent(const int *v, int count, int max, int *out) {
    for (int k = 0; k < count; ++k) out[k] = fe_clamp_extent(v[k], max);
}
// element offsets of image a's tables, as 64-bit numbers
void ih_kp_offset(const int *a, const int *i, int count, int k_max, unsigned long long *out) {
    for (int k = 0; k < count; ++k) out[k] = (unsigned long long)fe_kp_offset(a[k], k_max, i[k]);
}
void ih_depth_offset(const int *a, const int *yi, const int *xi, int count, int h_max, int w_max, unsigned long long *out) {
    for (int k = 0; k < count; ++k) out[k] = (unsigned long long)fe_depth_offset(a[k], h_max, w_max, yi[k], xi[k]);
}
}
