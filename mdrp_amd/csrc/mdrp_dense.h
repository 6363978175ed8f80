// mdrp_dense.h — the front end for DENSE matchers (include/mdrp_dense.h): from a warp (rows of (xA, yA, xB, yB)), its certainty and
// two depth maps to the estimators' padded float64 records, sampled by certainty on the device.
//
// mdrp_amd/frontend.py sample_dense_numpy is the definition (rules D1-D7).  Every quantity that decides a pick is an integer: the weight of a row
// (dense_weight, 1 .. 65536), the 24-bit stratum offset (dense_u), the position of pick k in the weights' running sum (dense_position) and the 4-D
// cell of a pick (dense_cell).  Sums of integers do not depend on the order a scan or an atomic adds them in, so the device result equals the NumPy
// one as bytes.  The first part of this file is host + device arithmetic (tests/hostmath/dense_host.cpp compiles it with a plain C++ compiler and
// pins it against frontend.py without a GPU); the kernels follow behind __HIPCC__:
//   k_dense_weights   D1-D3 for every row of the batch: the row's weight as the inclusive running sum INSIDE its block of DENSE_BLOCK_ROWS rows
//                     (uint32: a block sums to at most 2^26), the block's sum and its candidate count.  No full-length 64-bit prefix table exists.
//   k_dense_scan      one workgroup per pair: the block sums in place to their inclusive running sum (at most 4096 per pair), T, K and M1
//   k_dense_pick      D4 / D5, a lane per k: position, binary search over the block sums, binary search inside the block; a pick is a duplicate of
//                     its predecessor iff the predecessor's position is not below the picked row's start; ordered compaction inside the tile
//   k_dense_balance   D6, one workgroup per pair: the tiles' picks in order, the 4-D histogram in LDS (integer atomics), the stage-2 weights and
//                     their running sum, the stage-2 draw with its ordered compaction.  balanced = 0: the ordered stage-1 picks are the result.
//   k_dense_rank      ranked calls only: the rank of every final row by rank_key / rank_count of mdrp_prosac.h
//   k_dense_emit      D7: the record of every final row, at its position or (ranked) straight at its rank
#pragma once
#include <math.h>
#include <stdint.h>
#include "mdrp_frontend.h" // fe_pixel, fe_keep, fe_isfinite; under hipcc rank_key and rank_count as well

namespace mdrp {

constexpr int DENSE_NORMALIZED = 0, DENSE_PIXEL = 1; // == MDRP_DENSE_NORMALIZED, MDRP_DENSE_PIXEL
constexpr int DENSE_MAX_ROWS = 1 << 22;              // == MDRP_DENSE_MAX_ROWS: rows of a pair's warp
constexpr int DENSE_MAX_STAGE1 = 65536;              // == MDRP_DENSE_MAX_STAGE1: expansion * n
constexpr int DENSE_MAX_N = 16384;                   // == MDRP_DENSE_MAX_N
constexpr int DENSE_MAX_GRID = 8;                    // == MDRP_DENSE_MAX_GRID: the histogram has at most 8^4 = 4096 cells
constexpr uint32_t DENSE_ONE = 65536;                // the weight of a certainty above the threshold

// D1.  normalized: (v + 1) * (0.5 * extent) in float64 on the widened value, an add and then a multiply (nothing to contract); pixel: v itself.
MDRP_HD double dense_pixel_coord(double v, int extent, int coords) { return coords == DENSE_NORMALIZED ? (v + 1.0) * (0.5 * (double)extent) : v; }

// D2 (the certainty's part) and D3.  0: the certainty is not finite or not above zero, the row is no candidate.  Otherwise 1 .. 65536: the product with
// a power of two and the floor are exact, the clamp is made on the floating value (an overflowing product is +inf and clamps to 65536).
MDRP_HD uint32_t dense_weight(double c, double threshold) {
    if (!fe_isfinite(c) || !(c > 0.0)) return 0;
    const double cp = c > threshold ? 1.0 : c;
    const double f = floor(cp * 65536.0);
    return f >= 65536.0 ? DENSE_ONE : (f < 1.0 ? 1u : (uint32_t)f);
}

// D4.  The hash takes the seed, the stage and k, never the pair's position in the batch.
MDRP_HD uint32_t dense_lowbias32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
MDRP_HD uint32_t dense_u(uint32_t seed, uint32_t stage, uint32_t k) { return dense_lowbias32(seed * 0x9E3779B1u + stage * 0x85EBCA77u + k) >> 8; }
// position of pick k among weights that sum to S, for a draw of M: S <= 2^38, k < M <= 2^16, u < 2^24, every product stays below 2^63
MDRP_HD uint64_t dense_position(uint64_t k, uint64_t S, uint64_t M, uint32_t u) { return (k * S + (((uint64_t)u * S) >> 24)) / M; }

// D6.  The 4-D cell of a pick from its integer pixel indices alone (xi < w, yi < h: every factor is below grid), as one index below grid^4.
MDRP_HD int dense_cell(int xi1, int yi1, int xi2, int yi2, int w1, int h1, int w2, int h2, int grid) {
    const int a = (int)(((int64_t)xi1 * grid) / w1), b = (int)(((int64_t)yi1 * grid) / h1);
    const int c = (int)(((int64_t)xi2 * grid) / w2), d = (int)(((int64_t)yi2 * grid) / h2);
    return ((a * grid + b) * grid + c) * grid + d;
}
// the stage-2 weight of a pick whose cell holds `count` stage-1 picks (itself included: count >= 1)
MDRP_HD uint32_t dense_cell_weight(uint32_t count, uint32_t min_count) { return count >= min_count ? (1u << 20) / count : 1u; }

#if defined(__HIPCC__)

constexpr int DENSE_THREADS = 256;        // every kernel but k_dense_balance: four wavefronts
constexpr int DENSE_BLOCK_ROWS = 1024;    // rows per block sum: at most DENSE_MAX_ROWS / 1024 = 4096 blocks per pair
constexpr int DENSE_BAL_THREADS = 1024;   // k_dense_balance: sixteen wavefronts, one workgroup per pair
constexpr int DENSE_EMIT_RECORDS = RANK_THREADS * RANK_PER_THREAD; // records per workgroup of k_dense_rank
static_assert(DENSE_THREADS == RANK_THREADS, "k_dense_rank ranks with k_rank's counting loop");
static_assert(DENSE_MAX_STAGE1 / DENSE_THREADS == 256, "k_dense_balance holds 256 tile offsets");

// what the kernels take beside their scratch: the descriptor, flattened (m1_max = expansion * n, or n without balancing)
struct DenseArgs {
    const void *warp, *cert, *depth1, *depth2;
    const double *center1, *center2;
    int warp_type, cert_type, depth_type, coords, filter;
    int rows, h1, w1, h2, w2;
    int n, m1_max, grid, min_count, balanced, ranked;
    uint32_t seed;
    double threshold;
    int nblk, ntile; // blocks of DENSE_BLOCK_ROWS rows | tiles of DENSE_THREADS picks, per pair
};
struct DenseMeta {
    uint64_t T;      // sum of the weights
    uint32_t K, M1;  // candidates | stage-1 draws = min(m1_max, K)
};
// the call's scratch, a buffer of the handle carved per call.  Buffers that one thread writes and another thread of its workgroup reads behind a
// barrier are neither const nor __restrict__ in the kernels.
struct DenseScratch {
    uint32_t *qpre;   // [B][rows]           running sum of the weights inside the row's block
    uint64_t *bpre;   // [B][nblk]           block sums, then (k_dense_scan) their inclusive running sum
    uint32_t *bcnt;   // [B][nblk]           candidates per block
    DenseMeta *meta;  // [B]
    int32_t *cand;    // [B][ntile * 256]    stage-1 picks, compacted inside each tile
    int32_t *tcnt;    // [B][ntile]          picks kept per tile
    int32_t *p1;      // [B][m1_max]         stage-1 picks in order
    int32_t *cell;    // [B][m1_max]         their cells
    uint64_t *wpre;   // [B][m1_max]         running sum of the stage-2 weights
    int32_t *sel;     // [B][n]              the final rows, ascending
    int32_t *rank;    // [B][n]              ranked: the place of every final row in descending certainty
};

__device__ __forceinline__ double dense_ld(const void *p, int type, size_t at) { // (float -> double is exact)
    return type == FE_F32 ? (double)static_cast<const float *>(p)[at] : static_cast<const double *>(p)[at];
}

struct DenseRow {
    double p1x, p1y, p2x, p2y; // pixel coordinates (D1), not centred
    int xi1, yi1, xi2, yi2;
};
// D1 and rule 2 for row r of pair b: the pixel coordinates and whether both points are inside their maps
__device__ __forceinline__ bool dense_points(const DenseArgs &a, size_t b, int r, DenseRow &o) {
    const size_t at = 4 * (b * (size_t)a.rows + (size_t)r);
    o.p1x = dense_pixel_coord(dense_ld(a.warp, a.warp_type, at), a.w1, a.coords);
    o.p1y = dense_pixel_coord(dense_ld(a.warp, a.warp_type, at + 1), a.h1, a.coords);
    o.p2x = dense_pixel_coord(dense_ld(a.warp, a.warp_type, at + 2), a.w2, a.coords);
    o.p2y = dense_pixel_coord(dense_ld(a.warp, a.warp_type, at + 3), a.h2, a.coords);
    const bool in1 = fe_pixel(o.p1x, o.p1y, a.w1, a.h1, o.xi1, o.yi1), in2 = fe_pixel(o.p2x, o.p2y, a.w2, a.h2, o.xi2, o.yi2);
    return in1 && in2 && a.w1 > 0 && a.h1 > 0 && a.w2 > 0 && a.h2 > 0; // (a map without pixels has no row inside: -0.5 truncates to pixel 0, which it lacks)
}
// rule 3 for a row whose points are inside: yi < h, xi < w
__device__ __forceinline__ void dense_depths(const DenseArgs &a, size_t b, const DenseRow &o, double &e1, double &e2) {
    e1 = dense_ld(a.depth1, a.depth_type, (b * (size_t)a.h1 + (size_t)o.yi1) * (size_t)a.w1 + (size_t)o.xi1);
    e2 = dense_ld(a.depth2, a.depth_type, (b * (size_t)a.h2 + (size_t)o.yi2) * (size_t)a.w2 + (size_t)o.xi2);
}

// inclusive running sum over the lanes of a wavefront
template <typename T> __device__ __forceinline__ T dense_wave_scan(T v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// the smallest i in [0, len) with pre[i] > P; pre is non-decreasing and pre[len - 1] > P (len >= 1)
template <typename T> __device__ __forceinline__ int dense_search(const T *pre, int len, T P) {
    int lo = 0, hi = len - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] > P) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Grid (B, nblk).  A block of DENSE_BLOCK_ROWS rows in four coalesced passes of 256: each row's weight (two scattered depth reads for a row whose
// points are inside), the running sum inside the pass by wavefront shuffles and a 4-entry LDS table, the pass's total carried to the next one.
MDRP_GLOBAL __launch_bounds__(DENSE_THREADS) void k_dense_weights(DenseArgs a, uint32_t *__restrict__ qpre, uint64_t *__restrict__ bsum,
                                                                 uint32_t *__restrict__ bcnt) {
    __shared__ uint32_t s_sum[DENSE_THREADS / 64], s_cnt[DENSE_THREADS / 64];
    const size_t b = blockIdx.x;
    const int blk = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t base = 0, cands = 0;
    for (int j = 0; j < DENSE_BLOCK_ROWS / DENSE_THREADS; ++j) {
        const int r = blk * DENSE_BLOCK_ROWS + j * DENSE_THREADS + tid; // < 2^22 + 1024
        uint32_t q = 0;
        if (r < a.rows) {
            DenseRow o;
            if (dense_points(a, b, r, o)) {
                double e1, e2;
                dense_depths(a, b, o, e1, e2);
                if (fe_keep(e1, e2, a.filter)) q = dense_weight(dense_ld(a.cert, a.cert_type, b * (size_t)a.rows + (size_t)r), a.threshold);
            }
        }
        const uint32_t v = dense_wave_scan(q, lane);
        const int c = __popcll(__ballot(q > 0));
        if (lane == 63) s_sum[wave] = v;
        if (lane == 0) s_cnt[wave] = (uint32_t)c;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < DENSE_THREADS / 64; ++w) {
            before += w < wave ? s_sum[w] : 0;
            total += s_sum[w];
            cands += s_cnt[w];
        }
        if (r < a.rows) qpre[b * (size_t)a.rows + (size_t)r] = base + before + v;
        base += total;
        __syncthreads(); // the tables are rewritten by the next pass
    }
    if (tid == 0) {
        bsum[b * (size_t)a.nblk + blk] = base;
        bcnt[b * (size_t)a.nblk + blk] = cands;
    }
}

// One workgroup per pair: the block sums in place to their inclusive running sum.  A thread sums its run of consecutive blocks, thread 0 scans the
// 256 run totals, the thread walks its run again.  (bpre is read and written by the same thread only.)
MDRP_GLOBAL __launch_bounds__(DENSE_THREADS) void k_dense_scan(DenseArgs a, uint64_t *bpre, const uint32_t *__restrict__ bcnt, DenseMeta *__restrict__ meta) {
    __shared__ uint64_t s_run[DENSE_THREADS];
    __shared__ uint32_t s_cnt[DENSE_THREADS];
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int per = (a.nblk + DENSE_THREADS - 1) / DENSE_THREADS, lo = min(tid * per, a.nblk), hi = min(lo + per, a.nblk);
    uint64_t *pre = bpre + b * (size_t)a.nblk;
    const uint32_t *cnt = bcnt + b * (size_t)a.nblk;
    uint64_t sum = 0;
    uint32_t k = 0;
    for (int i = lo; i < hi; ++i) { sum += pre[i]; k += cnt[i]; }
    s_run[tid] = sum; s_cnt[tid] = k;
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0;
        uint32_t kk = 0;
        for (int t = 0; t < DENSE_THREADS; ++t) {
            const uint64_t v = s_run[t];
            s_run[t] = run; // exclusive
            run += v; kk += s_cnt[t];
        }
        DenseMeta m;
        m.T = run; m.K = kk; m.M1 = min((uint32_t)a.m1_max, kk);
        meta[b] = m;
    }
    __syncthreads();
    uint64_t run = s_run[tid];
    for (int i = lo; i < hi; ++i) { run += pre[i]; pre[i] = run; }
}

// Grid (B, ntile), a lane per k.  The kept picks of a tile go to the front of the tile's 256 slots in k order (ballot + popcount, a 4-entry LDS
// table); the tile's count goes to tcnt.  Picks are non-decreasing in k, so the tiles one behind the other are the ordered stage-1 picks.
MDRP_GLOBAL __launch_bounds__(DENSE_THREADS) void k_dense_pick(DenseArgs a, const uint32_t *__restrict__ qpre, const uint64_t *__restrict__ bpre,
                                                              const DenseMeta *__restrict__ meta, int32_t *__restrict__ cand, int32_t *__restrict__ tcnt) {
    __shared__ int s_wave[DENSE_THREADS / 64];
    const size_t b = blockIdx.x;
    const int tile = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const DenseMeta m = meta[b];
    const uint32_t k = (uint32_t)(tile * DENSE_THREADS + tid);
    bool keep = false;
    int row = -1;
    if (k < m.M1) { // M1 >= 1: a candidate exists, T >= 1; the position is below T
        const uint64_t P = dense_position(k, m.T, m.M1, dense_u(a.seed, 1, k));
        const uint64_t *pre = bpre + b * (size_t)a.nblk;
        const int blk = dense_search(pre, a.nblk, P);
        const uint64_t bstart = blk > 0 ? pre[blk - 1] : 0;
        const int r0 = blk * DENSE_BLOCK_ROWS, len = min(DENSE_BLOCK_ROWS, a.rows - r0);
        const uint32_t *q = qpre + b * (size_t)a.rows + (size_t)r0;
        const int i = dense_search(q, len, (uint32_t)(P - bstart)); // (P - bstart is below the block's sum <= 2^26)
        row = r0 + i;
        const uint64_t start = bstart + (i > 0 ? q[i - 1] : 0);
        keep = k == 0 || dense_position(k - 1, m.T, m.M1, dense_u(a.seed, 1, k - 1)) < start; // else the predecessor picked this row too
    }
    const unsigned long long ball = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(ball);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < DENSE_THREADS / 64; ++w) {
        const int c = s_wave[w];
        before += w < wave ? c : 0;
        total += c;
    }
    if (keep) cand[(b * (size_t)a.ntile + tile) * DENSE_THREADS + before + __popcll(ball & ((1ull << lane) - 1ull))] = row;
    if (tid == 0) tcnt[b * (size_t)a.ntile + tile] = total;
}

// One workgroup per pair.  The tiles' counts to offsets (at most 256, thread 0); balanced = 0: the tiles' picks one behind the other are the result.
// Otherwise every pick's cell is counted into the LDS histogram (grid^4 <= 4096 uint32, integer atomics), the stage-2 weights are summed in chunks
// of the workgroup's size with a carried base, and the stage-2 draw walks k in chunks with the ordered compaction of k_dense_pick and a carried count.
// Every loop bound is uniform over the workgroup.
MDRP_GLOBAL __launch_bounds__(DENSE_BAL_THREADS) void k_dense_balance(DenseArgs a, const int32_t *__restrict__ cand, const int32_t *__restrict__ tcnt,
                                                                     int32_t *p1, int32_t *cell, uint64_t *wpre, int32_t *__restrict__ sel,
                                                                     int32_t *__restrict__ n_out) {
    __shared__ uint32_t s_hist[DENSE_MAX_GRID * DENSE_MAX_GRID * DENSE_MAX_GRID * DENSE_MAX_GRID];
    __shared__ int s_toff[DENSE_MAX_STAGE1 / DENSE_THREADS + 1];
    __shared__ uint64_t s_sum[DENSE_BAL_THREADS / 64];
    __shared__ int s_cnt[DENSE_BAL_THREADS / 64];
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cells = a.grid * a.grid * a.grid * a.grid;
    cand += b * (size_t)a.ntile * DENSE_THREADS; tcnt += b * (size_t)a.ntile;
    p1 += b * (size_t)a.m1_max; cell += b * (size_t)a.m1_max; wpre += b * (size_t)a.m1_max; sel += b * (size_t)a.n;
    for (int t = tid; t < a.ntile; t += DENSE_BAL_THREADS) s_toff[t] = tcnt[t];
    for (int c = tid; c < cells; c += DENSE_BAL_THREADS) s_hist[c] = 0;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < a.ntile; ++t) {
            const int c = s_toff[t];
            s_toff[t] = run;
            run += c;
        }
        s_toff[a.ntile] = run;
    }
    __syncthreads();
    const int m1 = s_toff[a.ntile]; // <= M1 <= m1_max
    for (int at = tid; at < a.ntile * DENSE_THREADS; at += DENSE_BAL_THREADS) {
        const int t = at / DENSE_THREADS, j = at % DENSE_THREADS, i = s_toff[t] + j;
        if (i >= s_toff[t + 1]) continue;
        const int row = cand[at];
        if (!a.balanced) { sel[i] = row; continue; } // (m1_max = n here)
        DenseRow o;
        dense_points(a, b, row, o); // a candidate: its points are inside
        const int c = dense_cell(o.xi1, o.yi1, o.xi2, o.yi2, a.w1, a.h1, a.w2, a.h2, a.grid);
        atomicAdd(&s_hist[c], 1u);
        p1[i] = row; cell[i] = c;
    }
    if (!a.balanced) {
        if (tid == 0) n_out[b] = m1;
        return;
    }
    __syncthreads(); // the histogram, p1 and cell are the workgroup's from here on
    uint64_t S = 0;
    for (int i0 = 0; i0 < m1; i0 += DENSE_BAL_THREADS) {
        const int i = i0 + tid;
        const uint64_t w = i < m1 ? (uint64_t)dense_cell_weight(s_hist[cell[i]], (uint32_t)a.min_count) : 0;
        const uint64_t v = dense_wave_scan(w, lane);
        if (lane == 63) s_sum[wave] = v;
        __syncthreads();
        uint64_t before = 0, total = 0;
#pragma unroll
        for (int x = 0; x < DENSE_BAL_THREADS / 64; ++x) {
            before += x < wave ? s_sum[x] : 0;
            total += s_sum[x];
        }
        if (i < m1) wpre[i] = S + before + v;
        S += total;
        __syncthreads();
    }
    const uint32_t M2 = (uint32_t)min(a.n, m1);
    int kept = 0;
    for (uint32_t k0 = 0; k0 < M2; k0 += DENSE_BAL_THREADS) {
        const uint32_t k = k0 + (uint32_t)tid;
        bool keep = false;
        int i = 0;
        if (k < M2) { // m1 >= 1: S >= 1, the position is below S = wpre[m1 - 1]
            const uint64_t P = dense_position(k, S, M2, dense_u(a.seed, 2, k));
            i = dense_search((const uint64_t *)wpre, m1, P);
            const uint64_t start = i > 0 ? wpre[i - 1] : 0;
            keep = k == 0 || dense_position(k - 1, S, M2, dense_u(a.seed, 2, k - 1)) < start;
        }
        const unsigned long long ball = __ballot(keep);
        if (lane == 0) s_cnt[wave] = __popcll(ball);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int x = 0; x < DENSE_BAL_THREADS / 64; ++x) {
            const int c = s_cnt[x];
            before += x < wave ? c : 0;
            total += c;
        }
        if (keep) sel[kept + before + __popcll(ball & ((1ull << lane) - 1ull))] = p1[i]; // < M2 <= n: at most one slot per k
        kept += total;
        __syncthreads();
    }
    if (tid == 0) n_out[b] = kept;
}

// Grid (B, ceil(n / DENSE_EMIT_RECORDS)), launched for a ranked call only; a thread holds RANK_PER_THREAD record slots.  rank[j] of final row sel[j],
// j < count: its place among the pair's records in descending rank_key of the raw certainty, ties by ascending j, which is ascending row - k_rank's
// counting loop over the count keys (a NaN or a -0.0 cannot occur: a candidate's certainty is finite and above zero).
MDRP_GLOBAL __launch_bounds__(DENSE_THREADS) void k_dense_rank(const void *__restrict__ cert, int cert_type, int rows_per_pair, int n,
                                                              const int32_t *__restrict__ sel, const int32_t *__restrict__ n_out, int32_t *__restrict__ rank) {
    __shared__ uint64_t s_key[RANK_TILE];
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int m = min(max(n_out[b], 0), n);
    const int32_t *sel_b = sel + b * (size_t)n;
    const size_t c0 = b * (size_t)rows_per_pair;
    uint64_t key[RANK_PER_THREAD];
    int idx[RANK_PER_THREAD], cnt[RANK_PER_THREAD];
#pragma unroll
    for (int q = 0; q < RANK_PER_THREAD; ++q) {
        idx[q] = blockIdx.y * DENSE_EMIT_RECORDS + q * DENSE_THREADS + tid;
        key[q] = idx[q] < m ? rank_key(dense_ld(cert, cert_type, c0 + (size_t)sel_b[idx[q]])) : prosac::RANK_KEY_DROPPED;
        cnt[q] = 0;
    }
    rank_count(s_key, m, tid, [=](int j) { return rank_key(dense_ld(cert, cert_type, c0 + (size_t)sel_b[j])); }, key, idx, cnt);
#pragma unroll
    for (int q = 0; q < RANK_PER_THREAD; ++q)
        if (idx[q] < m) rank[b * (size_t)n + (size_t)idx[q]] = cnt[q]; // cnt < m: a permutation of [0, m)
}

// Grid (B, ceil(n / DENSE_THREADS)), a lane per record slot.  Slot j < count is final row sel[j]: its record is evaluated again from the warp and the
// maps and written at j, or (rank != null) at rank[j]: straight to its rank, there is no second copy of the records.  Slots at and past the count
// get the filler.
MDRP_GLOBAL __launch_bounds__(DENSE_THREADS) void k_dense_emit(DenseArgs a, const int32_t *__restrict__ sel, const int32_t *__restrict__ n_out,
                                                              const int32_t *__restrict__ rank, double *__restrict__ x1, double *__restrict__ x2,
                                                              double *__restrict__ d1, double *__restrict__ d2, int32_t *__restrict__ rows,
                                                              double *__restrict__ score) {
    const size_t b = blockIdx.x;
    const int j = blockIdx.y * DENSE_THREADS + threadIdx.x;
    if (j >= a.n) return;
    const int m = min(max(n_out[b], 0), a.n);
    size_t at = b * (size_t)a.n + (size_t)j;
    if (j < m) {
        const int row = sel[at];
        DenseRow o;
        dense_points(a, b, row, o); // a candidate: inside both maps
        double e1, e2;
        dense_depths(a, b, o, e1, e2);
        if (rank) at = b * (size_t)a.n + (size_t)rank[at]; // rank < m
        const double c1x = a.center1 ? a.center1[2 * b] : 0.0, c1y = a.center1 ? a.center1[2 * b + 1] : 0.0;
        const double c2x = a.center2 ? a.center2[2 * b] : 0.0, c2y = a.center2 ? a.center2[2 * b + 1] : 0.0;
        x1[2 * at] = o.p1x - c1x; x1[2 * at + 1] = o.p1y - c1y;
        x2[2 * at] = o.p2x - c2x; x2[2 * at + 1] = o.p2y - c2y;
        d1[at] = e1; d2[at] = e2;
        rows[at] = row;
        score[at] = dense_ld(a.cert, a.cert_type, b * (size_t)a.rows + (size_t)row);
    } else {
        x1[2 * at] = 0.0; x1[2 * at + 1] = 0.0;
        x2[2 * at] = 0.0; x2[2 * at + 1] = 0.0;
        d1[at] = 1.0; d2[at] = 1.0;
        rows[at] = -1;
        score[at] = 0.0;
    }
}

#endif // __HIPCC__

} // namespace mdrp
