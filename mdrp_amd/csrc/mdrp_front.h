// mdrp_front.h — the bar a hypothesis is retired against, and the bar a run's FIRST chunk builds for itself ("Retirement").
// A hypothesis matters only if it has more inliers or a lower MSAC score than every minimal model before it.  With `cand` an upper bound of its
// inlier count its score is at least thr (n - cand), so against records (rec_cnt, rec_score) that were reached BEFORE its iteration
//     cand <= rec_cnt   and   thr (n - cand) >= rec_score
// prove that it breaks neither.  Later chunks take the records the previous chunk ended with (struct Bar, mdrp_kernels.h).  The first chunk has
// none; but the records that a few of its own hypotheses (the picked set P, scored exactly first) reach at iterations strictly before t are no
// better than the true running records at t, so they are a valid bar for every other hypothesis of iteration t (prefix_bar).  Models of one
// iteration never serve as each other's bar: k_scan compares them one after the other.
// Plain C++ on both sides (MDRP_HD): tests/hostmath/front_host.cpp pins prefix_bar and RecordBar::retires against the sequential loop.
#pragma once
#include <cfloat>
#include <cstdint>
#include "mdrp_math.h"

namespace mdrp {

struct RecordBar {
    long long rec_cnt;
    double rec_score; // already inflated by 1e-12 relative; DBL_MAX: no record yet, nothing can be retired
    MDRP_HD RecordBar(long long cnt, double raw_score) : rec_cnt(cnt), rec_score(raw_score < DBL_MAX ? raw_score * (1.0 + 1e-12) : DBL_MAX) {}
    MDRP_HD bool armed() const { return rec_score < DBL_MAX; }
    // the bail-out predicate of the exact sweeps, for a hypothesis with `cnt` inliers and the sum `score` after `processed` of the pair's n records
    MDRP_HD bool out(int n, double thr, int processed, double score, int cnt) const {
        return ((long long)cnt + (long long)(n - processed) <= rec_cnt) && (score + thr * (double)(processed - cnt) >= rec_score);
    }
    // a hypothesis none of whose records has been looked at, with at most `cand` inliers: what k_count and the first chunk's filter test
    MDRP_HD bool retires(int n, double thr, int cand) const { return !((long long)cand > rec_cnt || thr * (double)(n - cand) < rec_score); }
};

// The records of the picked hypotheses of iterations strictly before `iter`: (max count, min score) over the entries with iter_p < iter and a
// count (cnt_p >= 0: a slot the sweep's own bail-out retired holds -2 and sets no record).  None: (-1, DBL_MAX), which retires nothing.
MDRP_HD RecordBar prefix_bar(const int32_t *iter_p, const int32_t *cnt_p, const double *score_p, int np, int iter) {
    long long rc = -1;
    double rs = DBL_MAX;
    for (int j = 0; j < np; ++j) {
        if (iter_p[j] < iter && cnt_p[j] >= 0) {
            if ((long long)cnt_p[j] > rc) rc = cnt_p[j];
            if (score_p[j] < rs) rs = score_p[j];
        }
    }
    return RecordBar(rc, rs);
}

// k_count hands a hypothesis on with its candidate density: key = min(64, ceil(64 cand / n)).  The most candidates a key stands for.
MDRP_HD int cand_of_key(int key, int n) { return (int)(((long long)key * n) >> 6); }

} // namespace mdrp
