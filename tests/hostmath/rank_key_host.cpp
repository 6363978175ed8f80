// Host build of the ranking key (mdrp_amd/csrc/mdrp_prosac.h, rank_key) for tests/test_frontend_ranked_host.py: plain C entry points over
// arrays, no GPU.  g++ -O2 -std=c++17 -fPIC -shared rank_key_host.cpp -o librank_key_host.so
#include "../../mdrp_amd/csrc/mdrp_prosac.h"

using namespace mdrp::prosac;

extern "C" {

void rk_keys_f64(const double *s, int count, uint64_t *key) {
    for (int k = 0; k < count; ++k) key[k] = rank_key(s[k]);
}
// a float score as the kernels take it: widened to double, then the same key
void rk_keys_f32(const float *s, int count, uint64_t *key) {
    for (int k = 0; k < count; ++k) key[k] = rank_key((double)s[k]);
}
uint64_t rk_key_dropped(void) { return RANK_KEY_DROPPED; }
}
