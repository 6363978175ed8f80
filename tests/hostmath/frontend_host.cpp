// Host build of the front end's per-row rules (mdrp_amd/csrc/mdrp_frontend.h) for tests/test_frontend_host.py: plain C entry points over
// arrays, no GPU.  g++ -O2 -std=c++17 -fPIC -shared frontend_host.cpp -o libfrontend_host.so
#include "../../mdrp_amd/csrc/mdrp_frontend.h"

using namespace mdrp;

extern "C" {

// in[k] = the coordinate is inside a w x h map, xi / yi its pixel (0 where outside)
void fh_pixel_f32(const float *x, const float *y, int count, int w, int h, int *in, int *xi, int *yi) {
    for (int k = 0; k < count; ++k) in[k] = fe_pixel(x[k], y[k], w, h, xi[k], yi[k]) ? 1 : 0;
}
void fh_pixel_f64(const double *x, const double *y, int count, int w, int h, int *in, int *xi, int *yi) {
    for (int k = 0; k < count; ++k) in[k] = fe_pixel(x[k], y[k], w, h, xi[k], yi[k]) ? 1 : 0;
}
void fh_keep(const double *d1, const double *d2, int count, int filter, int *keep) {
    for (int k = 0; k < count; ++k) keep[k] = fe_keep(d1[k], d2[k], filter) ? 1 : 0;
}
void fh_row_valid(const int *i, const int *j, int count, int k1, int k2, int *ok) {
    for (int k = 0; k < count; ++k) ok[k] = fe_row_valid(i[k], j[k], k1, k2) ? 1 : 0;
}
int fh_filter_both_inf(void) { return FE_FILTER_BOTH_INF; }
int fh_filter_finite(void) { return FE_FILTER_FINITE; }
}
