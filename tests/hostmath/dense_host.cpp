// Host build of the dense front end's arithmetic (mdrp_amd/csrc/mdrp_dense.h: D1, D3, the hash, the position of a pick, the cell index) for
// tests/test_dense_host.py: the same text the kernels compile, called on arrays.  Test scaffolding, not product code.
//   g++ -O2 -std=c++17 -fPIC -shared dense_host.cpp -o libdense_host.so
#include "../../mdrp_amd/csrc/mdrp_dense.h"

using namespace mdrp;

extern "C" {

void dh_pixel_f32(const float *v, int count, int extent, int coords, double *out) {
    for (int i = 0; i < count; ++i) out[i] = dense_pixel_coord((double)v[i], extent, coords);
}
void dh_pixel_f64(const double *v, int count, int extent, int coords, double *out) {
    for (int i = 0; i < count; ++i) out[i] = dense_pixel_coord(v[i], extent, coords);
}
void dh_weight_f32(const float *c, int count, double threshold, uint32_t *out) {
    for (int i = 0; i < count; ++i) out[i] = dense_weight((double)c[i], threshold);
}
void dh_weight_f64(const double *c, int count, double threshold, uint32_t *out) {
    for (int i = 0; i < count; ++i) out[i] = dense_weight(c[i], threshold);
}
void dh_lowbias32(const uint32_t *x, int count, uint32_t *out) {
    for (int i = 0; i < count; ++i) out[i] = dense_lowbias32(x[i]);
}
void dh_u(uint64_t seed, uint32_t stage, const uint32_t *k, int count, uint32_t *out) {
    for (int i = 0; i < count; ++i) out[i] = dense_u((uint32_t)seed, stage, k[i]); // the low 32 bits of the seed, as the entry points take them
}
void dh_position(const uint64_t *k, const uint32_t *u, int count, uint64_t S, uint64_t M, uint64_t *out) {
    for (int i = 0; i < count; ++i) out[i] = dense_position(k[i], S, M, u[i]);
}
void dh_cell(const int32_t *xi1, const int32_t *yi1, const int32_t *xi2, const int32_t *yi2, int count, int w1, int h1, int w2, int h2, int grid, int32_t *out) {
    for (int i = 0; i < count; ++i) out[i] = dense_cell(xi1[i], yi1[i], xi2[i], yi2[i], w1, h1, w2, h2, grid);
}
void dh_cell_weight(const uint32_t *cnt, int count, uint32_t min_count, uint32_t *out) {
    for (int i = 0; i < count; ++i) out[i] = dense_cell_weight(cnt[i], min_count);
}
void dh_limits(int *out) { // rows, expansion * n, n, grid; coords
    out[0] = DENSE_MAX_ROWS; out[1] = DENSE_MAX_STAGE1; out[2] = DENSE_MAX_N; out[3] = DENSE_MAX_GRID; out[4] = DENSE_NORMALIZED; out[5] = DENSE_PIXEL;
}

} // extern "C"
