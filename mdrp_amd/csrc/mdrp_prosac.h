// mdrp_prosac.h — estimate in match-score order (mdrp_estimate_batch_ranked, include/mdrp.h).
//
// PROSAC as the reference's RandomSampler draws it (initialize_prosac @0x4f8a20, generate_sample): while sample index k < max_prosac_iterations
// a sample is K - 1 distinct draws from the first subset - 1 records plus record subset - 1, and the subset grows by the growth table; from
// sample max_prosac_iterations on it is the uniform draw of K from n (K = 3 for the monodepth estimators, 5 / 6 / 7 for the baselines of
// mdrp_classic.h: the sample size is a parameter of everything below).  The sequence is a pure function of (seed, n, K, max_prosac_iterations), and
// the subset size of a sample does not depend on the RNG at all: the host builds one schedule per distinct n (subset_schedule below) and
// k_samples_prosac reads it.  Everything else of a ranked call is the unchanged estimator, run on the records in descending score order:
//   k_rank              scores -> order (one workgroup per pair, rank by counting, scores tiled through LDS: one path for every n; rank_key and
//                       rank_count are shared with the ranked front end, k_gather_ranked / k_gather_images_ranked of mdrp_frontend.h)
//   k_rank_gather       x1, x2, d1, d2 -> handle-owned copies in that order, in front of the unchanged estimate_device (a baseline has no depths:
//                       the depth pointers are null and nothing of them is read or written)
//   k_samples_prosac    the wave-speculative sampler (samples_block, mdrp_kernels.h) with a variable number of raw draws per sample
//   k_rank_scatter      the inlier mask back into the caller's order, behind the run
//
// The first part is host-only C++17 without a device header (tests/hostmath/prosac_host.cpp pins it against the reference's tables without a GPU).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace mdrp {
namespace prosac {

constexpr int K = 3; // sample size of the monodepth estimators; the 5- / 6- / 7-point baselines pass theirs (mdrp_estimate_classic_ranked)

// RandomSampler::initialize_prosac: growth[i] = samples after which the subset may grow past i + 1 records, for samples of `ssz` records.  fp64, one
// operation per step, in this order (no contraction: there is no multiply-add pair here to contract).
inline std::vector<uint64_t> growth_table(uint64_t n, uint64_t max_prosac_iterations, int ssz = K) {
    std::vector<uint64_t> growth(std::max<uint64_t>(n, (uint64_t)ssz), 1);
    if (n < (uint64_t)ssz) return growth;
    double T = (double)max_prosac_iterations;
    for (int i = 0; i < ssz; ++i) {
        const double ratio = (double)(ssz - i) / (double)(n - (uint64_t)i);
        T = T * ratio;
    }
    uint64_t Tp = 1;
    for (uint64_t i = (uint64_t)ssz; i < n; ++i) {
        const double num = T * ((double)i + 1.0);
        const double Tn = num / ((double)i + 1.0 - (double)ssz);
        const double step = std::ceil(Tn - T);
        Tp = (uint64_t)((double)Tp + step);
        growth[i] = Tp;
        T = Tn;
    }
    return growth;
}

// samples [0, prosac_samples) are drawn progressively, every later one uniformly (generate_sample tests sample_k < max_prosac_iterations with
// sample_k starting at 1)
inline uint64_t prosac_samples(uint64_t max_prosac_iterations) { return max_prosac_iterations > 0 ? max_prosac_iterations - 1 : 0; }

// subset size of sample j for j = 0 .. min(count, prosac_samples) - 1, by replaying generate_sample's bookkeeping (at most one growth step per
// sample).  With `truncate` the table ends where the subset has reached n: every progressive sample behind the table's end draws from all n.
inline std::vector<uint32_t> subset_schedule(uint64_t n, uint64_t max_prosac_iterations, uint64_t count, bool truncate, int ssz = K) {
    std::vector<uint32_t> sub_of;
    if (n < (uint64_t)ssz) return sub_of;
    const std::vector<uint64_t> growth = growth_table(n, max_prosac_iterations, ssz);
    uint64_t k = 1, sub = (uint64_t)ssz;
    for (uint64_t j = 0; j < count && k < max_prosac_iterations; ++j) {
        if (truncate && sub >= n) break;
        sub_of.push_back((uint32_t)sub);
        ++k;
        if (k < max_prosac_iterations && k > growth[sub - 1]) sub = std::min<uint64_t>(sub + 1, n);
    }
    return sub_of;
}

// ------------------------------------------------------------------------------------------------ ranking key
#if defined(__HIPCC__)
#define MDRP_PROSAC_HD __host__ __device__ __forceinline__
#else
#define MDRP_PROSAC_HD inline
#endif

// The key of a score as an unsigned integer that orders like the definition: NaN -> -inf, -0.0 -> +0.0, then the usual monotone map of the
// IEEE bits (negative: all bits flipped; otherwise: the sign bit set).  Larger key = better score.  The smallest key is that of -inf,
// 0x000fffffffffffff: 0 is below every key (the ranked front end, mdrp_frontend.h, gives it to the rows it drops).  Host and device
// (tests/hostmath/rank_key_host.cpp pins it on the CPU); the bits are taken through a union, as mdrp_frontend.h takes them.
MDRP_PROSAC_HD uint64_t rank_key(double s) {
    union { double f; uint64_t u; } v;
    v.f = s;
    uint64_t b = v.u;
    const uint64_t mag = b & 0x7fffffffffffffffULL;
    if (mag > 0x7ff0000000000000ULL) b = 0xfff0000000000000ULL; // NaN (either sign, any payload) -> -inf
    else if (mag == 0) b = 0;                                    // -0.0 -> +0.0
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
constexpr uint64_t RANK_KEY_DROPPED = 0; // below rank_key(-inf)

} // namespace prosac
} // namespace mdrp

#if defined(__HIPCC__)
#include "mdrp_kernels.h"
#include "mdrp_classic.h"

namespace mdrp {

// ------------------------------------------------------------------------------------------------ sampler
// samples_block with K - 1 raw draws per progressive sample and K per uniform one.  One body for every sample size: k_samples_prosac is its K = 3
// kernel (the monodepth estimators, main unit; tests/test_prosac_resources.py reads its budget by that name), kc_samples_prosac<K> its kernels for the
// baselines' K = 5, 6, 7, instantiated with their other kernels (mdrp_instances.h).  Sample j of the table is progressive iff j < n_prosac; with P progressive samples
// left at the start of a step, thread i speculates that its sample starts (K-1) min(i, P) + K max(0, i - P) draws behind the workgroup's state.
// Threads up to and including the first one that redrew a duplicate are right, the step commits those.  The table carries (RNG state, sample
// index) across chunks: table_state, table_k.  A progressive sample is K - 1 distinct draws from the first sub - 1 records (draw_sample_k's
// duplicate rule) and record sub - 1.  While the subset is barely larger than K almost every sample redraws and a step commits few samples: the
// first ~60 samples of a table cost about as many steps (DESIGN.md 7e gives the measured time).
template <int K>
__device__ __forceinline__ void samples_prosac_tables(int n_tables, const int32_t *__restrict__ table_n, uint64_t *__restrict__ table_state,
                                                      uint64_t *__restrict__ table_k, const uint64_t *__restrict__ sub_off /*[n_tables + 1]*/,
                                                      const uint32_t *__restrict__ sub_of, uint64_t n_prosac, int chunk_len,
                                                      uint32_t *__restrict__ samples /*[n_tables][chunk_len][K]*/) {
    __shared__ int s_first[SAMP_THREADS / 64];
    __shared__ unsigned long long s_state;
    const uint64_t GAMMA = 0x9e3779b97f4a7c15ULL;
    const int t = blockIdx.x;
    if (t >= n_tables) return;
    const uint64_t n = (uint64_t)table_n[t];
    if (n < (uint64_t)K) return;
    uint64_t state = table_state[t];
    const uint64_t j0 = table_k[t];
    __syncthreads(); // every thread holds the state before thread 0 advances it
    const uint32_t *tab = sub_of + sub_off[t];
    const uint64_t tab_len = sub_off[t + 1] - sub_off[t];
    uint32_t *out = samples + (size_t)t * chunk_len * K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, nwaves = nthreads >> 6;
    int done = 0;
    while (done < chunk_len) {
        const uint64_t jb = j0 + (uint64_t)done;               // sample index of thread 0
        const uint64_t P = jb < n_prosac ? n_prosac - jb : 0;  // progressive samples left
        const uint64_t i = (uint64_t)tid, pre = i < P ? i : P;
        uint64_t s = state + ((uint64_t)(K - 1) * pre + (uint64_t)K * (i - pre)) * GAMMA;
        const uint64_t s0 = s;
        uint32_t smp[K];
        uint64_t expect;
        if (i < P) {
            const uint64_t j = jb + i;
            const uint64_t sub = j < tab_len ? (uint64_t)tab[j] : n; // (>= K: the first sub - 1 >= K - 1 records hold K - 1 distinct indices)
            const uint64_t m = sub - 1;
            draw_sample_k<K - 1>(m, s, smp);
            smp[K - 1] = (uint32_t)m;
            expect = K - 1;
        } else {
            draw_sample_k<K>(n, s, smp);
            expect = K;
        }
        const bool rejected = (s - s0) != expect * GAMMA;
        const unsigned long long ball = __ballot(rejected);
        if (lane == 0) s_first[wave] = ball ? wave * 64 + (__ffsll((long long)ball) - 1) : SAMP_THREADS;
        __syncthreads();
        int first = nthreads - 1;
        for (int w = nwaves - 1; w >= 0; --w) { const int v = s_first[w]; if (v < SAMP_THREADS) first = v; }
        const int nvalid = min(first + 1, chunk_len - done);
        if (tid < nvalid) {
#pragma unroll
            for (int k = 0; k < K; ++k) out[(size_t)K * (done + tid) + k] = smp[k];
        }
        if (tid == nvalid - 1) s_state = s;
        __syncthreads();
        state = s_state;
        done += nvalid;
    }
    if (tid == 0) { table_state[t] = state; table_k[t] = j0 + (uint64_t)chunk_len; }
}
MDRP_GLOBAL __launch_bounds__(SAMP_THREADS) void k_samples_prosac(int n_tables, const int32_t *__restrict__ table_n, uint64_t *__restrict__ table_state,
                                                                 uint64_t *__restrict__ table_k, const uint64_t *__restrict__ sub_off,
                                                                 const uint32_t *__restrict__ sub_of, uint64_t n_prosac, int chunk_len,
                                                                 uint32_t *__restrict__ samples /*[n_tables][chunk_len][3]*/) {
    samples_prosac_tables<3>(n_tables, table_n, table_state, table_k, sub_off, sub_of, n_prosac, chunk_len, samples);
}
template <int K>
__global__ __launch_bounds__(SAMP_THREADS) void kc_samples_prosac(int n_tables, const int32_t *__restrict__ table_n, uint64_t *__restrict__ table_state,
                                                                  uint64_t *__restrict__ table_k, const uint64_t *__restrict__ sub_off,
                                                                  const uint32_t *__restrict__ sub_of, uint64_t n_prosac, int chunk_len,
                                                                  uint32_t *__restrict__ samples /*[n_tables][chunk_len][K]*/) {
    samples_prosac_tables<K>(n_tables, table_n, table_state, table_k, sub_off, sub_of, n_prosac, chunk_len, samples);
}

// ------------------------------------------------------------------------------------------------ ranking
using prosac::rank_key;

constexpr int RANK_THREADS = 256, RANK_PER_THREAD = 4, RANK_TILE = 2048;

// The counting loop of k_rank and of the ranked front end (k_gather_ranked, mdrp_frontend.h): cnt[q] += #{j in [0, n) : key_j > key[q], or
// key_j == key[q] and j < idx[q]} for the RANK_PER_THREAD records a thread holds, key_j = load(j) read by the workgroup into LDS tiles of
// RANK_TILE and broadcast from there.  Every thread of the workgroup calls it with the same n: the barriers are the tile's.
template <typename Load>
__device__ __forceinline__ void rank_count(uint64_t *s_key /*LDS, RANK_TILE*/, int n, int tid, const Load &load, const uint64_t (&key)[RANK_PER_THREAD],
                                           const int (&idx)[RANK_PER_THREAD], int (&cnt)[RANK_PER_THREAD]) {
    for (int t0 = 0; t0 < n; t0 += RANK_TILE) {
        const int tl = min(RANK_TILE, n - t0);
        __syncthreads(); // the tile's readers of the previous round are done
        for (int j = tid; j < tl; j += RANK_THREADS) s_key[j] = load(t0 + j);
        __syncthreads();
        for (int j = 0; j < tl; ++j) {
            const uint64_t kj = s_key[j];
#pragma unroll
            for (int q = 0; q < RANK_PER_THREAD; ++q) cnt[q] += (kj > key[q] || (kj == key[q] && t0 + j < idx[q])) ? 1 : 0;
        }
    }
}

// One workgroup per pair.  rank of record i = records that come before it = #{j : key_j > key_i, or key_j == key_i and j < i} (a stable descending
// sort); order[rank] = i.  Each thread ranks RANK_PER_THREAD records per pass against all n keys, read as LDS broadcasts from tiles of RANK_TILE
// keys.  order[r] = -1 for r in [n, n_max).
MDRP_GLOBAL __launch_bounds__(RANK_THREADS) void k_rank(const double *__restrict__ scores /*[batch][n_max]*/, const int32_t *__restrict__ n_per_pair,
                                                       int n_max, int32_t *__restrict__ order /*[batch][n_max]*/) {
    __shared__ uint64_t s_key[RANK_TILE];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(n_per_pair[pair], 0), n_max);
    const double *sc = scores + (size_t)pair * n_max;
    int32_t *ord = order + (size_t)pair * n_max;
    for (int r = n + tid; r < n_max; r += RANK_THREADS) ord[r] = -1;
    for (int base = 0; base < n; base += RANK_THREADS * RANK_PER_THREAD) {
        uint64_t key[RANK_PER_THREAD];
        int idx[RANK_PER_THREAD], cnt[RANK_PER_THREAD];
#pragma unroll
        for (int q = 0; q < RANK_PER_THREAD; ++q) {
            idx[q] = base + q * RANK_THREADS + tid;
            key[q] = idx[q] < n ? rank_key(sc[idx[q]]) : 0;
            cnt[q] = 0;
        }
        rank_count(s_key, n, tid, [sc](int j) { return rank_key(sc[j]); }, key, idx, cnt);
#pragma unroll
        for (int q = 0; q < RANK_PER_THREAD; ++q)
            if (idx[q] < n) ord[cnt[q]] = idx[q]; // (cnt < n: a permutation of [0, n))
    }
}

// records of pair blockIdx.x in rank order into the ordered copies; rows at or past n are zero.  d1o null (a baseline call): no depths, d1 / d2 / d2o are not touched
MDRP_GLOBAL __launch_bounds__(256) void k_rank_gather(const int32_t *__restrict__ order, const int32_t *__restrict__ n_per_pair, int n_max,
                                                     const double *__restrict__ x1, const double *__restrict__ x2, const double *__restrict__ d1,
                                                     const double *__restrict__ d2, double *__restrict__ x1o, double *__restrict__ x2o,
                                                     double *__restrict__ d1o, double *__restrict__ d2o) {
    const int pair = blockIdx.x, r = blockIdx.y * 256 + threadIdx.x;
    if (r >= n_max) return;
    const int n = min(max(n_per_pair[pair], 0), n_max);
    const size_t o = (size_t)pair * n_max;
    double2 a = make_double2(0.0, 0.0), b = a;
    double u = 0.0, v = 0.0;
    if (r < n) {
        const int src = order[o + r];
        if (src >= 0 && src < n) {
            a = reinterpret_cast<const double2 *>(x1)[o + src]; b = reinterpret_cast<const double2 *>(x2)[o + src];
            if (d1o) { u = d1[o + src]; v = d2[o + src]; }
        }
    }
    reinterpret_cast<double2 *>(x1o)[o + r] = a; reinterpret_cast<double2 *>(x2o)[o + r] = b;
    if (d1o) { d1o[o + r] = u; d2o[o + r] = v; }
}

// mask[order[r]] = mask_ranked[r] for r < n; bytes at or past n are zero.  order is a permutation of [0, n): every byte is written once.
MDRP_GLOBAL __launch_bounds__(256) void k_rank_scatter(const int32_t *__restrict__ order, const int32_t *__restrict__ n_per_pair, int n_max,
                                                      const uint8_t *__restrict__ mask_ranked, uint8_t *__restrict__ mask) {
    const int pair = blockIdx.x, r = blockIdx.y * 256 + threadIdx.x;
    if (r >= n_max) return;
    const int n = min(max(n_per_pair[pair], 0), n_max);
    const size_t o = (size_t)pair * n_max;
    if (r >= n) { mask[o + r] = 0; return; }
    const int dst = order[o + r];
    if (dst >= 0 && dst < n) mask[o + dst] = mask_ranked[o + r];
}

} // namespace mdrp
#endif
