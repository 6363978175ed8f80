// Host build of the first chunk's front (tests/test_front_host.py): the solver's LDS reservation rule (mdrp_amd/csrc/mdrp_schedule.h) and the
// prefix-record retirement predicate (mdrp_amd/csrc/mdrp_front.h) as plain C entry points, no GPU.
// g++ -O2 -std=c++17 -fPIC -shared front_host.cpp -o libfront_host.so
#include "../../mdrp_amd/csrc/mdrp_front.h"
#include "../../mdrp_amd/csrc/mdrp_schedule.h"

extern "C" {

uint64_t fh_solver_reservation(uint64_t lds_per_cu, int resident_per_simd, uint64_t keep_free) {
    return (uint64_t)mdrp::sched::solver_reservation((size_t)lds_per_cu, resident_per_simd, (size_t)keep_free);
}
int fh_first_pick(int kind, int batch_call, int wave_max_pairs, int knob) { return mdrp::sched::first_pick(kind, batch_call, wave_max_pairs, knob); }
int fh_cand_of_key(int key, int n) { return mdrp::cand_of_key(key, n); }
// k_first_filter's decision for a hypothesis of iteration `iter` with at most `cand` inliers, against the picked table (iter_p, cnt_p, score_p)[np]
int fh_retires(const int32_t *iter_p, const int32_t *cnt_p, const double *score_p, int np, int iter, int n, double thr, int cand) {
    return mdrp::prefix_bar(iter_p, cnt_p, score_p, np, iter).retires(n, thr, cand) ? 1 : 0;
}
// the chunk-start test of k_count against raw records
int fh_bar_retires(long long rec_cnt, double rec_score, int n, double thr, int cand) { return mdrp::RecordBar(rec_cnt, rec_score).retires(n, thr, cand) ? 1 : 0; }
}
