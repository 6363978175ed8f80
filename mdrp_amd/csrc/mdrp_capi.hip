// mdrp_capi.hip — C ABI (include/mdrp.h) and host orchestration of the chunked, phase-split LO-RANSAC.
// Everything numerical runs in the gfx950 kernels of mdrp_kernels.h; the host only sizes buffers, groups pairs by
// correspondence count (one sample table per distinct N) and reads back one 16-byte progress record per chunk.
#include "../../include/mdrp.h"
#include "mdrp_kernels.h"
#include "mdrp_classic.h"
#include "mdrp_frontend.h"
#include "mdrp_schedule.h"
#include "mdrp_from_model.h"
#include "mdrp_prior.h"
#include "mdrp_prosac.h"
#include "mdrp_classic_models.h"
#include "mdrp_classic_focals.h"
#include "mdrp_dense.h"
#include "mdrp_reconstruct.h"
#include "mdrp_scene.h"
#include "mdrp_covis.h"
#include "mdrp_fuse.h"
// MDRP_SPLIT_TU (the default build): the k_final family, k_from_model, k_prior, kc_from_model, kc_prior and the baselines' kernels are instantiated in mdrp_tu.hip, compiled in parallel with
// this file; a single-unit build (experiment builds with -D switches: mdrp_amd/build.py single=True) instantiates them here, implicitly.
#ifdef MDRP_SPLIT_TU
#define MDRP_INST extern
#include "mdrp_instances.h"
namespace mdrp {
MDRP_INSTANCES_FINAL_64
MDRP_INSTANCES_FINAL_256
MDRP_INSTANCES_CLASSIC
MDRP_INSTANCES_FROM_MODEL
MDRP_INSTANCES_PRIOR
MDRP_INSTANCES_CLASSIC_MODELS
}
#endif

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

using namespace mdrp;

static_assert(sizeof(mdrp_model) == sizeof(Model), "model layout");
static_assert(sizeof(mdrp_camera) == sizeof(CamDev), "camera layout");
static_assert(sizeof(mdrp_result) == sizeof(ResultDev), "result layout");
static_assert(sizeof(mdrp_focal_pose) == sizeof(FocalPose) && offsetof(mdrp_focal_pose, votes) == offsetof(FocalPose, votes) &&
              offsetof(mdrp_focal_pose, status) == offsetof(FocalPose, status), "focal pose layout");
static_assert(MDRP_FOCAL_NO_MODEL == FOCAL_NO_MODEL && MDRP_FOCAL_F1_NOT_REAL == FOCAL_F1_NOT_REAL && MDRP_FOCAL_F2_NOT_REAL == FOCAL_F2_NOT_REAL &&
              MDRP_FOCAL_NO_VOTERS == FOCAL_NO_VOTERS, "status bits of the header and of the kernel");

namespace {

// The thread's last error message.  Every failure of the library assigns it on its way out, and nothing else does: `raised` is how a call's scope
// (MDRP_ENTER) knows that the call is failing, whichever return statement it leaves through.
struct LastError {
    std::string msg;
    bool raised = false;
    LastError &operator=(std::string m) { msg = std::move(m); raised = true; return *this; }
    const char *c_str() const { return msg.c_str(); }
};
thread_local LastError g_err;

#define HIPCHK(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) {                                                                            \
            char buf_[512];                                                                                \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            g_err = buf_;                                                                                  \
            return MDRP_ERR_HIP;                                                                           \
        }                                                                                                  \
    } while (0)

// device memory of a handle: grows on demand, freed with the handle
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return MDRP_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        // grow with headroom so alternating sizes do not thrash
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { g_err = std::string("hipMalloc failed: ") + hipGetErrorString(e); p = nullptr; return MDRP_ERR_HIP; }
        cap = want;
        return MDRP_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// One DevBuf carved into a call's blocks, each 16-byte aligned: take() every block's bytes, ensure() the buffer, then at<T>() a block.
struct Carve {
    size_t total = 0;
    unsigned char *base = nullptr;
    size_t take(size_t bytes) { const size_t at = total; total += (bytes + 15) & ~(size_t)15; return at; }
    int ensure(DevBuf &buf, size_t least = 0) {
        if (int rc = buf.ensure(std::max(total, least))) return rc;
        base = buf.as<unsigned char>();
        return MDRP_OK;
    }
    template <typename T> T *at(size_t offset) const { return reinterpret_cast<T *>(base + offset); }
};

// any other HIP object of a handle (stream, event, pinned host memory): destroyed with the handle, or when creating the handle fails half-way
template <typename T, auto Destroy> struct Owned {
    T v = nullptr;
    Owned() = default;
    Owned(Owned &&o) noexcept : v(o.v) { o.v = nullptr; }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }
    void reset() { if (v) (void)Destroy(v); v = nullptr; }
    operator T() const { return v; }
    T operator->() const { return v; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
template <typename T> using Pinned = Owned<T *, hipHostFree>;

// read back once per super-chunk
struct Progress {
    int32_t n_active, pad_;         // (pad_ keeps max_needed 8-byte aligned)
    unsigned long long max_needed;
    unsigned long long evals;       // (model x correspondence) evaluations the CPU loop would do: sum over pairs of models * n
    unsigned long long evals_mfma;  // evaluations executed by k_count on the matrix cores (padded to 16 x 16 tiles)
    unsigned long long evals_sweep; // evaluations handed to the fp64 sweep (survivors * n)
    unsigned long long evals_bound; // evaluations executed by k_bound in fp32 (k_count's survivors * n)
    int32_t wish_sum, wish_pairs;   // final refinements: sum over the pairs of first_chunk_wish(inlier ratio of the result), number of pairs (RunParams::inl_stat)
};
// the `counters` buffer, zeroed at the start of every super-chunk
struct Counters {
    int32_t unused_[2];
    Progress progress;
    int32_t lo_head[16];                 // queue head of the super-chunk's LO launch, in a 64-byte block of its own
    int32_t xcd_head[8 * LO_XCD_STRIDE]; // per-XCD LO queue heads, LO_XCD_STRIDE ints apart (lo_take, mdrp_kernels.h)
};
static_assert(offsetof(Counters, progress) == 2 * sizeof(int32_t) && offsetof(Counters, lo_head) == 16 * sizeof(int32_t) &&
              offsetof(Counters, xcd_head) == 32 * sizeof(int32_t) && sizeof(Counters) == 640, "counter block layout");
static_assert(offsetof(Progress, evals_mfma) == offsetof(Progress, evals) + sizeof(unsigned long long), "k_count adds to stats[0] and stats[1]");
static_assert(offsetof(Progress, wish_pairs) == offsetof(Progress, wish_sum) + sizeof(int32_t), "RunParams::inl_stat is [2]");
constexpr size_t LM_STATS_BYTES = 6 * sizeof(unsigned long long); // mdrp_handle::lm_stats

// Every entry point runs on the handle's device and puts the caller's current device back on return (the caller is
// usually torch, which tracks its own current device).
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) ok = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

} // namespace

struct mdrp_handle {
    std::mutex mu; // one call at a time per handle (scratch, events and counters are per handle); different handles run concurrently
    int device = 0;
    hipStream_t stream = nullptr;      // the caller's (null: the device's legacy default stream) or own_stream
    Stream own_stream;
    Stream aux_stream;                 // the second chunk's sampler + solver run here, beside the first chunk's sweep
    Stream aux_stream2;                // the sample tables and the super-chunk's LO launch run here
    Stream copy_stream;                // host-buffer calls: the H2D slices of the correspondences
    Event ev_copied, ev_prepped, ev_solved6;
    DevBuf fuse;                       // fused tail: control words (64 B) | done_cnt[batch] | fin_done[batch] | ready[batch]
    Event ev_lo, ev_tables, ev_sampled[2], ev_solved[sched::NC_MAX], ev_scanned[sched::NC_MAX]; // per chunk of a super-chunk
    int num_cu = 256;
    size_t lds_per_cu = 65536; // LDS of a compute unit, from the device properties (sched::solver_reservation)
    // persistent device buffers
    DevBuf pts, dep, st;
    DevBuf params;                     // per-call parameters in ONE upload: table states | cameras | table sizes | table of pair | n per pair
    Pinned<unsigned char> params_host; // staging of the same
    size_t params_host_cap = 0;
    DevBuf models, slot_score, slot_inl, triggers, work_pair, counters, results, mask, plan;
    // [c & 1]: chunk c of a super-chunk (chunk c + 1 is solved beside the sweep of chunk c)
    DevBuf samples[2], tags[2], model_count[2];
    DevBuf tags_sorted[2]; // survivor lists ordered by candidate density (k_sort_tags)
    DevBuf tags_v, surv_count; // survivors of k_count (unsorted, with density keys) and their number per pair
    DevBuf cand_stat; // [2 batch] u64: candidates | evaluations of the run's first chunk per pair (k_count's split point)
    DevBuf und_count; // k_count's two phases: hypotheses phase A left undecided, per pair (stride 2); the list itself and the partial counts alias the sorted tag lists
    DevBuf rfrag;              // MFMA A fragments of the correspondences (k_prep): [pair][ceil(n_max/16)][64] x 16 B
    DevBuf cplan;              // work plan of k_count / k_bound
    DevBuf surv2_count;        // survivors of k_bound per pair
    DevBuf lo_mask;            // 5-point LO: inlier subset of the refined model, one row per LO workgroup
    DevBuf red5;               // 5-point solver: the Reduce5 blocks between its kernels, [pair][ceil(chunk / 64)][76][64] doubles, + a region for the first chunk (PassScratch)
    DevBuf lm_stats;                  // six u64: correspondences evaluated by the LM cost / accumulate sweeps of the LO kernel | of the final kernel |
                                      // fused tail: gate time-outs | final-refinement wait time-outs
    Pinned<unsigned long long> lm_stats_host; // copy, valid after finish_timing
    int64_t fuse_gate_timeouts = 0, fuse_wait_timeouts = 0; // of the last call
    int64_t first_chunk = 0;                                // of the last call (mdrp_stats::first_chunk)
    double seen_wish[3] = {-1.0, -1.0, -1.0};               // per monodepth estimator: mean first_chunk_wish over the results of its last call that measured it
    Pinned<int32_t> wish_host; Event ev_wish;               // unfused runs: the two sums are copied behind the final refinements and read by the next call
    int wish_kind = -1;                                     // ... of this estimator, once ev_wish has completed (-1: nothing pending)
    bool fuse_disabled = false;       // a bounded wait of the fused tail expired on this handle: streams do not overlap here, run unfused ...
    int fuse_retry_in = 0;            // ... for this many API calls, then try the fused tail again (a busy moment on a shared GPU is not a profiler)
    int fuse_backoff = 64;            // ... doubled after every consecutive expired wait (capped), reset by a call whose fused tail ran through
    // budgets call (mdrp_estimate_batch_budgets): per pass the checkpoint states [C][pairs] and problem list | representatives | done flags
    // ([C][pairs] int32 each); per call the result planes [C][batch] and, where the caller gives no device mask, the mask planes [C][batch][n_max]
    DevBuf ckpt, ck_list, bresults, bmask;
    int last_budgets = 0;              // budgets of the last call (0: it had none)
    DevBuf in_x1, in_x2, in_d1, in_d2; // staging when the caller passes host memory
    DevBuf fm_models, fm_init;         // mdrp_refine_batch (and mdrp_estimate_batch_prior: the priors): the caller's models when they come from host memory | start-model scores [batch] f64, counts [batch] i32
    // ranked calls (mdrp_estimate_batch_ranked): the correspondences in score order | order [batch][n_max] int32 | the mask in that order |
    // scores and n per pair when they come from host memory | per pass: sample index per table (u64) | schedule offsets (u64, tables + 1) | subset sizes (u32)
    DevBuf pr_x1, pr_x2, pr_d1, pr_d2, pr_order, pr_mask, pr_scores, pr_nper, pr_tab;
    DevBuf fe_key;                     // ranked front end (k_gather_ranked): the key of every match row, [batch][m_max] uint64
    DevBuf fe_x1, fe_x2, fe_d1, fe_d2, fe_slot, fe_n; // device front end (mdrp_estimate_matches_async): gathered correspondences | slot of every match row | kept rows per pair
    Pinned<int32_t> fe_n_host;         // the counts, read by the host scheduler
    size_t fe_n_host_cap = 0;
    DevBuf fp_nper, fp_in, fp_out;     // focals and pose from F (include/mdrp_classic_focals.h): n per pair | a host call's models, mask and principal points | its records
    DevBuf dn_scratch, dn_score;       // dense front end (include/mdrp_dense.h): the sampler's scratch, carved per call (DenseScratch) | mdrp_estimate_dense_async: the records' certainties
    // back end, carved per call (calls on a handle are serialised on one stream, and every word a kernel reads was written by its own call) -
    // clouds (include/mdrp_reconstruct.h): the pairs' ReconPair | the two camera tables | tile counts; co-visibility (include/mdrp_covis.h): the pairs'
    // CovisPair | the two camera tables; scenes (include/mdrp_scene.h): the images' records (where the caller takes none) | their SceneImage | the
    // camera table | tile counts
    DevBuf be_scratch;
    DevBuf unit_a, unit_b, unit_c, unit_d, unit_e, unit_f;
    Pinned<Progress> progress_host;
    // sweep timing
    std::vector<std::pair<Event, Event>> ev_pool;
    std::vector<int> ev_what; // 0 = k_score (fp64 sweep), 1 = k_count (MFMA), 2 = LO, 3 = final refinement, 4 = k_bound, 5 = minimal solver
    size_t ev_used = 0;
    double sweep_ms = 0.0, count_ms = 0.0;
    double kind_ms[6] = {0, 0, 0, 0, 0, 0};
    int64_t kind_launches[6] = {0, 0, 0, 0, 0, 0};
    int64_t lm_cost_evals = 0, lm_accum_evals = 0, fin_cost_evals = 0, fin_accum_evals = 0;
    int64_t count_launches = 0;
    int64_t sweep_launches = 0, sweep_evals = 0, mfma_evals = 0, fp64_evals = 0, bound_evals = 0;
    int last_batch = 0;
    // the start of an estimator or refine call: what the fetch entry points will accept, and the counters of mdrp_last_stats at zero
    void begin_call(int batch, int n_budgets) {
        last_batch = batch; last_budgets = n_budgets;
        ev_used = 0; sweep_ms = 0; count_ms = 0; sweep_launches = 0; count_launches = 0;
        sweep_evals = 0; mfma_evals = 0; fp64_evals = 0; bound_evals = 0; lm_cost_evals = 0; lm_accum_evals = 0;
    }
};

namespace {

// one LM instantiation per kernel: dispatch (kind, estimate_shift) on the host
#define MDRP_LM_DISPATCH_T(KERNEL, T, kind, shift, grid, smem, stream, ...)                                          \
    do {                                                                                                             \
        if ((kind) == 0 && (shift)) hipLaunchKernelGGL((KERNEL<0, true, T>), grid, dim3(T), smem, stream, __VA_ARGS__);  \
        else if ((kind) == 0) hipLaunchKernelGGL((KERNEL<0, false, T>), grid, dim3(T), smem, stream, __VA_ARGS__);       \
        else if ((kind) == 1) hipLaunchKernelGGL((KERNEL<1, false, T>), grid, dim3(T), smem, stream, __VA_ARGS__);       \
        else hipLaunchKernelGGL((KERNEL<2, false, T>), grid, dim3(T), smem, stream, __VA_ARGS__);                        \
    } while (0)
// threads per LM problem: one wavefront (64) when problems outnumber SIMDs, a 256-thread workgroup otherwise
#define MDRP_LM_DISPATCH(KERNEL, threads, kind, shift, grid, smem, stream, ...)                                      \
    do {                                                                                                             \
        if ((threads) == 64) MDRP_LM_DISPATCH_T(KERNEL, 64, kind, shift, grid, smem, stream, __VA_ARGS__);           \
        else MDRP_LM_DISPATCH_T(KERNEL, 256, kind, shift, grid, smem, stream, __VA_ARGS__);                          \
    } while (0)

// k_final: the user's loss type of the inlier-only refinement is a template parameter as well (rp.final_loss): one instantiation per loss type of
// BundleOptions (an unknown type is the TRIVIAL loss, as in loss_value)
#define MDRP_FINAL_DISPATCH_L(T, FL, kind, shift, grid, smem, stream, ...)                                                  \
    do {                                                                                                                   \
        if ((kind) == 0 && (shift)) hipLaunchKernelGGL((k_final<0, true, T, FL>), grid, dim3(T), smem, stream, __VA_ARGS__);  \
        else if ((kind) == 0) hipLaunchKernelGGL((k_final<0, false, T, FL>), grid, dim3(T), smem, stream, __VA_ARGS__);       \
        else if ((kind) == 1) hipLaunchKernelGGL((k_final<1, false, T, FL>), grid, dim3(T), smem, stream, __VA_ARGS__);       \
        else hipLaunchKernelGGL((k_final<2, false, T, FL>), grid, dim3(T), smem, stream, __VA_ARGS__);                        \
    } while (0)
#define MDRP_FINAL_DISPATCH_T(T, floss, kind, shift, grid, smem, stream, ...)                                               \
    do {                                                                                                                   \
        switch (floss) {                                                                                                   \
        case 1: MDRP_FINAL_DISPATCH_L(T, 1, kind, shift, grid, smem, stream, __VA_ARGS__); break;                          \
        case 2: MDRP_FINAL_DISPATCH_L(T, 2, kind, shift, grid, smem, stream, __VA_ARGS__); break;                          \
        case 3: MDRP_FINAL_DISPATCH_L(T, 3, kind, shift, grid, smem, stream, __VA_ARGS__); break;                          \
        case 4: MDRP_FINAL_DISPATCH_L(T, 4, kind, shift, grid, smem, stream, __VA_ARGS__); break;                          \
        case 5: MDRP_FINAL_DISPATCH_L(T, 5, kind, shift, grid, smem, stream, __VA_ARGS__); break;                          \
        default: MDRP_FINAL_DISPATCH_L(T, 0, kind, shift, grid, smem, stream, __VA_ARGS__); break; /* TRIVIAL, like loss_value's default */ \
        }                                                                                                                  \
    } while (0)
#define MDRP_FINAL_DISPATCH(threads, floss, kind, shift, grid, smem, stream, ...)                                           \
    do {                                                                                                                   \
        if ((threads) == 64) MDRP_FINAL_DISPATCH_T(64, floss, kind, shift, grid, smem, stream, __VA_ARGS__);               \
        else MDRP_FINAL_DISPATCH_T(256, floss, kind, shift, grid, smem, stream, __VA_ARGS__);                              \
    } while (0)

// scoring sweeps: pose models with cheirality (calibrated monodepth, 5-point), F = diag(1,1,f2) E diag(1,1,f1) (focal estimators),
// or a raw fundamental matrix in the model's first nine doubles (7-point)
#define MDRP_SWEEP_DISPATCH(KERNEL, kind, grid, block, smem, stream, ...)                                                       \
    do {                                                                                                                        \
        if ((kind) == MDRP_CALIB || (kind) == MDRP_RELPOSE_5PT) hipLaunchKernelGGL((KERNEL<true, false>), grid, block, smem, stream, __VA_ARGS__); \
        else if ((kind) == MDRP_FUNDAMENTAL_7PT) hipLaunchKernelGGL((KERNEL<false, true>), grid, block, smem, stream, __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<false, false>), grid, block, smem, stream, __VA_ARGS__);                                 \
    } while (0)
// classic LM kernels: (kind, threads per problem)
#define MDRP_CLASSIC_LM_DISPATCH(KERNEL, threads, kind, grid, smem, stream, ...)                                                 \
    do {                                                                                                                        \
        if ((kind) == MDRP_RELPOSE_5PT && (threads) == 64) hipLaunchKernelGGL((KERNEL<CLASSIC_RELPOSE, 64>), grid, dim3(64), smem, stream, __VA_ARGS__); \
        else if ((kind) == MDRP_RELPOSE_5PT) hipLaunchKernelGGL((KERNEL<CLASSIC_RELPOSE, 256>), grid, dim3(256), smem, stream, __VA_ARGS__); \
        else if ((kind) == MDRP_SHARED_6PT && (threads) == 64) hipLaunchKernelGGL((KERNEL<CLASSIC_SHARED, 64>), grid, dim3(64), smem, stream, __VA_ARGS__); \
        else if ((kind) == MDRP_SHARED_6PT) hipLaunchKernelGGL((KERNEL<CLASSIC_SHARED, 256>), grid, dim3(256), smem, stream, __VA_ARGS__); \
        else if ((threads) == 64) hipLaunchKernelGGL((KERNEL<CLASSIC_FUND, 64>), grid, dim3(64), smem, stream, __VA_ARGS__);      \
        else hipLaunchKernelGGL((KERNEL<CLASSIC_FUND, 256>), grid, dim3(256), smem, stream, __VA_ARGS__);                        \
    } while (0)

int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
}
bool front_clear_on() { return env_int("MDRP_FRONT_CLEAR", 1) != 0; } // (read by estimate_device and by its passes)

// LDS work lists: 2 buffers of u16 indices, stride = n_max rounded to 64 (0 disables the lists)
int lm_list_stride(int n_max) { return n_max <= LM_LIST_MAX_N ? ((n_max + 63) / 64) * 64 : 0; }
size_t lm_list_bytes(int n_max) { return (size_t)2 * lm_list_stride(n_max) * sizeof(uint16_t); }
// k_final: a third list (the indices a record mask lets through, lm_mask_index) while the three stay within 32 KiB of dynamic LDS
int lm_mask_index_on(int n_max) { return lm_list_stride(n_max) > 0 && (size_t)3 * lm_list_stride(n_max) * sizeof(uint16_t) <= 32768 ? 1 : 0; }
size_t lm_final_list_bytes(int n_max) { return (size_t)(2 + lm_mask_index_on(n_max)) * lm_list_stride(n_max) * sizeof(uint16_t); }

int get_events(mdrp_handle *h, hipEvent_t *a, hipEvent_t *b, int what = 0) {
    if (h->ev_used == h->ev_pool.size()) {
        Event x, y;
        HIPCHK(hipEventCreate(&x.v));
        HIPCHK(hipEventCreate(&y.v));
        h->ev_pool.emplace_back(std::move(x), std::move(y));
        h->ev_what.push_back(0);
    }
    h->ev_what[h->ev_used] = what;
    *a = h->ev_pool[h->ev_used].first;
    *b = h->ev_pool[h->ev_used].second;
    h->ev_used++;
    return MDRP_OK;
}

int solver_for(int kind, int est_shift) {
    if (kind == MDRP_CALIB) return est_shift ? SOLVER_SHIFT : SOLVER_P3P;
    return kind == MDRP_SHARED_FOCAL ? SOLVER_SHARED : SOLVER_VARYING;
}

// Every buffer of handle h that a pass allocates, with its bytes: a Pass ensures exactly these, estimate_device sizes its passes from them.
// `lead0`: the first leading chunk of the run's first super-chunk (0: none).
struct PassScratch {
    std::vector<std::pair<DevBuf *, size_t>> bufs;
    size_t fuse; // (ensured by the super-chunk that runs the fused tail)
    // `params`: table states | cameras 1 | cameras 2 | table sizes | table of pair | n per pair | budgets (a budgets call: MAX_BUDGETS u64)
    size_t params, off_cam1, off_cam2, off_tn, off_tof, off_nper, off_bud;
    // Reduce5 blocks of the 5-point solver (Pass::solve): [pair][ceil(len / 64)] blocks of RED5_STRIDE x 64 doubles per solve, in two regions.
    // The first chunk of a super-chunk of several chunks is solved on the main stream while the second chunk's solver may run on `aux` (the
    // sliced host-buffer front: the main stream waits for a slice's k_prep only, not for the solver issued behind it), so it gets a region of
    // its own behind the shared one.  Its length is a leading chunk that leaves at least as much again behind it: at most lead0 and
    // chunk_cap / 2 iterations.
    size_t red5_blocks, red5_first_blocks; // per pair
    size_t total() const {
        size_t t = fuse;
        for (const auto &b : bufs) t += b.second;
        return t;
    }
};

PassScratch pass_scratch(mdrp_handle *h, int kind, int batch, int n_max, int n_tables, int chunk_cap, uint64_t lead0, int n_budgets = 0) {
    const size_t b = (size_t)batch, n = (size_t)n_max, t = (size_t)n_tables, slots = b * chunk_cap * sched::model_slots(kind);
    PassScratch z;
    z.fuse = 64 + 3 * sizeof(int32_t) * b;
    z.off_cam1 = sizeof(uint64_t) * t; z.off_cam2 = z.off_cam1 + sizeof(CamDev) * b; z.off_tn = z.off_cam2 + sizeof(CamDev) * b;
    z.off_tof = z.off_tn + sizeof(int32_t) * t; z.off_nper = z.off_tof + sizeof(int32_t) * b;
    z.off_bud = (z.off_nper + sizeof(int32_t) * b + 7) / 8 * 8; z.params = n_budgets ? z.off_bud + sizeof(uint64_t) * MAX_BUDGETS : z.off_nper + sizeof(int32_t) * b;
    z.red5_blocks = ((size_t)chunk_cap + 63) / 64;
    z.red5_first_blocks = (std::min<uint64_t>(lead0, (uint64_t)chunk_cap / 2) + 63) / 64;
    const size_t samples = sizeof(uint32_t) * sched::sample_size(kind) * t * chunk_cap, tags = sizeof(uint32_t) * slots, pair2 = sizeof(int32_t) * 2 * b;
    z.bufs = { // (in the order of allocation: params_host is allocated behind params)
        {&h->pts, sizeof(double) * PT_STRIDE * b * n}, {&h->dep, kind >= MDRP_RELPOSE_5PT ? 0 : sizeof(double) * 2 * b * n}, {&h->st, sizeof(PairState) * b},
        {&h->samples[0], samples}, {&h->params, z.params},
        {&h->models, sizeof(Model) * slots}, {&h->slot_score, sizeof(double) * slots}, {&h->slot_inl, sizeof(int32_t) * slots},
        {&h->tags[0], tags}, {&h->model_count[0], pair2}, {&h->model_count[1], pair2}, {&h->tags[1], tags}, {&h->tags_sorted[0], tags},
        {&h->tags_sorted[1], tags}, {&h->samples[1], samples}, {&h->tags_v, tags},
        {&h->surv_count, sizeof(int32_t) * b}, {&h->cand_stat, sizeof(unsigned long long) * 2 * b}, {&h->und_count, pair2},
        {&h->cplan, sizeof(int32_t) * (b + 1)}, {&h->surv2_count, sizeof(int32_t) * b},
        {&h->rfrag, std::max<size_t>(1024, b * ((n + 15) / 16) * 1024)},
        {&h->triggers, sizeof(Trigger) * b * chunk_cap},     // worst case: every iteration triggers
        {&h->work_pair, sizeof(int32_t) * (3 * b + 2)},      // LO plan of a super-chunk: prefix | begin | end | total
        {&h->counters, sizeof(Counters)},
        {&h->plan, sizeof(int32_t) * (2 * b + 2 + 4 + 16)}, // k_plan's two prefix arrays (batch + 1 each) | its totals {dense, total, head} | spare
        // the 5- and 6-point LO keeps the inlier subset of the model it refines: one row per LO workgroup (kc_lo launches num_cu * (8 | 2) of them)
        {&h->lo_mask, (kind == MDRP_RELPOSE_5PT || kind == MDRP_SHARED_6PT) ? (size_t)h->num_cu * 8 * std::max<size_t>(n, 1) : 0},
        {&h->red5, kind == MDRP_RELPOSE_5PT ? sizeof(double) * b * (z.red5_blocks + z.red5_first_blocks) * RED5_STRIDE * 64 : 0},
        {&h->ckpt, sizeof(PairState) * b * n_budgets}, {&h->ck_list, sizeof(int32_t) * 3 * b * n_budgets}};
    return z;
}

// the caller's HOST buffers of a pass
struct HostSrc { const double *x1, *x2, *d1, *d2; };
// a budgets call: the budgets and, for this pass, row 0 of its pairs in the result and mask planes ([n][plane] records, [n][plane][n_max] bytes)
struct BudgetOut { const uint64_t *budgets; int n; ResultDev *results; uint8_t *mask; int plane; };

// strictly increasing budgets >= 1, at most MAX_BUDGETS, the last one the run's max_iterations: checked before any device work
int check_budgets(const mdrp_ransac_opt *ro, const uint64_t *budgets, int n_budgets) {
    const char *why = nullptr;
    if (!ro || !budgets || n_budgets < 1) why = "budgets: an empty list";
    else if (n_budgets > MAX_BUDGETS) why = "budgets: more than MDRP_MAX_BUDGETS";
    else {
        for (int c = 0; c < n_budgets && !why; ++c)
            if (budgets[c] < 1 || (c > 0 && budgets[c] <= budgets[c - 1])) why = "budgets: must be >= 1 and strictly increasing";
        if (!why && budgets[n_budgets - 1] != ro->max_iterations) why = "budgets: ransac_opt.max_iterations must equal the last budget";
    }
    if (why) { g_err = why; return MDRP_ERR_INVALID; }
    return MDRP_OK;
}
// the one n_per_pair range check (n_per_pair null: n_max for every pair)
const char *n_per_pair_out_of_range(const int32_t *n_per_pair, int batch, int n_max) {
    for (int i = 0; n_per_pair && i < batch; ++i)
        if (n_per_pair[i] < 0 || n_per_pair[i] > n_max) return "n_per_pair out of range";
    return nullptr;
}
constexpr int HOST_SLICE_PAIRS = 256; // pairs per H2D slice of a host-buffer call (24.6 MB at N = 2000: ~0.5 ms of PCIe per slice)

// one pass = a contiguous range of pairs that fits the scratch budget: what estimate_device hands run_pass (pointers offset to the pass's first pair)
struct PassIn {
    int kind;
    const double *x1, *x2, *d1, *d2; // device memory; with `host`, the handle's staging buffers, still to be filled
    int batch, n_max;
    const int32_t *n_host;
    const mdrp_camera *cam1, *cam2;
    const mdrp_ransac_opt *ro;
    const mdrp_bundle_opt *bo;
    int chunk_cap;
    uint8_t *mask_dev;
    ResultDev *results_dev;
    const HostSrc *host;  // (or null)
    int batch_call;       // pairs of the whole API call
    const BudgetOut *bud; // (or null)
    const Model *priors;  // device memory, one per pair of the pass, or null (mdrp_estimate_batch_prior, mdrp_estimate_classic_prior; never with `host` or `bud`)
    int prior_space;      // the baselines' priors: 0 = the caller's units, 1 = the estimator's normalised coordinates (include/mdrp_classic_models.h)
    const uint64_t *prosac; // ranked call: max_prosac_iterations of the progressive sampler (mdrp_prosac.h), or null: the uniform sampler
    bool clear_lm_stats;    // the call's first pass, where estimate_device has left the LM statistics to the pass's front clear (Pass::clear_front)
};

// One estimator call, as its entry point describes it to estimate_device (and, with the caller's models beside it, to the refine calls).  Every
// default means "not used": an entry point names what it uses and nothing else.
struct EstimateCall {
    int kind = -1;
    const double *x1 = nullptr, *x2 = nullptr, *d1 = nullptr, *d2 = nullptr; // device memory; with `host`, the handle's staging buffers, still to be filled
    int batch = 0, n_max = 0;
    const int32_t *n_per_pair = nullptr;          // host memory, or null: n_max for every pair
    const mdrp_camera *cam1 = nullptr, *cam2 = nullptr;
    const mdrp_ransac_opt *ro = nullptr;
    const mdrp_bundle_opt *bo = nullptr;
    uint8_t *mask_dev = nullptr;                  // the caller's device mask, or null: the handle's (its planes, in a budgets call)
    const HostSrc *host = nullptr;                // the sliced host front (mdrp_estimate_batch[_budgets] on host buffers): run_pass issues the copies
    const uint64_t *budgets = nullptr; int n_budgets = 0;
    const Model *priors = nullptr; int prior_space = 0; // PassIn::priors, [batch] in device memory, and PassIn::prior_space
    const uint64_t *prosac = nullptr;             // PassIn::prosac
};

// the pairs [p0, p0 + nb) of a call as a pass: every per-pair pointer offset by p0 (`n_host`, `mask`, `hs` and `bud` are the pass's already)
PassIn pass_in(mdrp_handle *h, const EstimateCall &c, int p0, int nb, const int32_t *n_host, int chunk_cap, uint8_t *mask, const HostSrc *hs, const BudgetOut *bud) {
    const size_t o1 = (size_t)p0 * c.n_max, o2 = 2 * o1;
    PassIn in{};
    in.kind = c.kind; in.batch = nb; in.n_max = c.n_max; in.batch_call = c.batch; in.chunk_cap = chunk_cap;
    in.x1 = c.x1 + o2; in.x2 = c.x2 + o2; in.d1 = c.d1 ? c.d1 + o1 : nullptr; in.d2 = c.d2 ? c.d2 + o1 : nullptr;
    in.n_host = n_host;
    in.cam1 = c.cam1 ? c.cam1 + p0 : nullptr; in.cam2 = c.cam2 ? c.cam2 + p0 : nullptr;
    in.ro = c.ro; in.bo = c.bo;
    in.mask_dev = mask; in.results_dev = h->results.as<ResultDev>() + p0;
    in.host = hs; in.bud = bud;
    in.priors = c.priors ? c.priors + p0 : nullptr; in.prior_space = c.prior_space; in.prosac = c.prosac;
    return in;
}

// The progressive sampler's launch for samples of `ssz` records (3, or the baselines' 5 / 6 / 7): Pass::samples and mdrp_prosac_samples[_k] both go
// through here.  `tab`: sample index per table | schedule offsets | subset sizes (prosac_tables).
struct ProsacTab { uint64_t *k; const uint64_t *off; const uint32_t *sub; };
void launch_samples_prosac(hipStream_t st, int ssz, int threads, int n_tables, const int32_t *d_table_n, uint64_t *d_table_state, const ProsacTab &tab,
                           uint64_t max_prosac, int len, uint32_t *smp) {
#define MDRP_PROSAC_LAUNCH(KERNEL)                                                                                                                \
    hipLaunchKernelGGL(KERNEL, dim3(n_tables), dim3(threads), 0, st, n_tables, d_table_n, d_table_state, tab.k, tab.off, tab.sub,                  \
                       prosac::prosac_samples(max_prosac), len, smp)
    if (ssz == 5) MDRP_PROSAC_LAUNCH(kc_samples_prosac<5>);
    else if (ssz == 6) MDRP_PROSAC_LAUNCH(kc_samples_prosac<6>);
    else if (ssz == 7) MDRP_PROSAC_LAUNCH(kc_samples_prosac<7>);
    else MDRP_PROSAC_LAUNCH(k_samples_prosac);
#undef MDRP_PROSAC_LAUNCH
}
// the tables of a run of at most `count` samples, one schedule per sample table, uploaded on `s` (pageable staging: the copy has left it on return)
int prosac_tables(mdrp_handle *h, hipStream_t s, int ssz, const int32_t *tab_n, int n_tables, uint64_t max_prosac, uint64_t count, ProsacTab &tab) {
    std::vector<uint64_t> head(2 * (size_t)n_tables + 1, 0); // k = 0 per table | offsets
    std::vector<uint32_t> sub;
    for (int t = 0; t < n_tables; ++t) {
        const std::vector<uint32_t> one = prosac::subset_schedule((uint64_t)std::max(tab_n[t], 0), max_prosac, count, true, ssz);
        head[n_tables + t] = sub.size();
        sub.insert(sub.end(), one.begin(), one.end());
    }
    head[2 * (size_t)n_tables] = sub.size();
    const size_t hb = sizeof(uint64_t) * head.size(), sb = sizeof(uint32_t) * sub.size();
    if (int rc = h->pr_tab.ensure(hb + sb + 16)) return rc;
    unsigned char *d = h->pr_tab.as<unsigned char>();
    HIPCHK(hipMemcpyAsync(d, head.data(), hb, hipMemcpyHostToDevice, s));
    if (sb) HIPCHK(hipMemcpyAsync(d + hb, sub.data(), sb, hipMemcpyHostToDevice, s));
    tab.k = reinterpret_cast<uint64_t *>(d); tab.off = tab.k + n_tables; tab.sub = reinterpret_cast<const uint32_t *>(d + hb);
    return MDRP_OK;
}

// The k_scan instantiation of a chunk, by the model slots per sample and the chunk's length (four iterations per lane where a 4-slot chunk is
// long: a 9872-iteration chunk is 39 steps of one wavefront instead of 154).  The scheduler (Pass::scan) and mdrp_replay_slots both launch through
// here.  Returns 10 * MPS + IPL of the instantiation it launched.
int launch_scan(hipStream_t s, int mps, int pairs, const RunParams &r, PairState *st, const double *slot_score, const int32_t *slot_inl, Trigger *trig,
                int trig_cap, const int32_t *model_count, unsigned long long *scan_stats) {
#define MDRP_SCAN(M, I)                                                                                                                            \
    do {                                                                                                                                           \
        hipLaunchKernelGGL((k_scan<M, I>), dim3(pairs), dim3(64), 0, s, r, st, slot_score, slot_inl, trig, trig_cap, model_count, scan_stats);      \
        return 10 * M + I;                                                                                                                         \
    } while (0)
    if (mps == 16) MDRP_SCAN(16, 1);
    if (mps == 12) MDRP_SCAN(12, 1);
    if (r.chunk_len >= 1024) MDRP_SCAN(4, 4);
    MDRP_SCAN(4, 1);
#undef MDRP_SCAN
}
// ... and of a chunk that was swept against a bar, from the sweep's sorted tag lists (k_scan_list; `list_cap` candidates per pair at most, pairs
// with more are walked as above by the same instantiation)
void launch_scan_list(hipStream_t s, int mps, int pairs, const RunParams &r, PairState *st, const double *slot_score, const int32_t *slot_inl, Trigger *trig,
                      int trig_cap, const int32_t *model_count, const uint32_t *tags_sorted, int list_cap, unsigned long long *scan_stats) {
    const int cap = std::min(std::max(list_cap, 0), SCAN_LIST_MAX);
#define MDRP_SCAN_LIST(M, I) \
    hipLaunchKernelGGL((k_scan_list<M, I>), dim3(pairs), dim3(SCAN_LIST_THREADS), 0, s, r, st, slot_score, slot_inl, trig, trig_cap, model_count, tags_sorted, cap, scan_stats)
    if (mps == 16) MDRP_SCAN_LIST(16, 1);
    else if (mps == 12) MDRP_SCAN_LIST(12, 1);
    else if (r.chunk_len >= 1024) MDRP_SCAN_LIST(4, 4);
    else MDRP_SCAN_LIST(4, 1);
#undef MDRP_SCAN_LIST
}

// Chunk c of the super-chunk under way, for the pairs [p0, p0 + pc).  Every kernel of the front indexes its per-pair arrays as base[pair]: a RANGE
// of pairs is the same launch on offset bases with r.batch = pc (the plans are per-launch scratch).  The whole batch is the range [0, batch); the
// host-buffer front runs the first chunk and the second chunk's solver slice by slice while later slices are still on their way over PCIe.
// Chunks alternate between two sets of tag lists / model counters / sample tables ([c & 1]); slots and triggers of different chunks are disjoint.
struct ChunkView {
    int c, p0, pc;
    bool first_of_run; // no records yet: nothing to retire against
    RunParams r;       // the pass's, with chunk_len, chunk_off and batch of this view
    PairState *st;
    double *pts, *dep, *slot_score;
    Model *models;
    int32_t *slot_inl, *model_count, *surv1, *surv2, *und_count;
    uint32_t *samples, *tags, *tags_sorted, *tags_sorted_other, *tags_v;
    unsigned long long *cand_stat;
    uint4 *rfrag;
    Trigger *trig;
};
// what goes on to a chunk's exact sweep: k_count's survivors, k_bound's, or what the first chunk's filter kept
struct Survivors { const uint32_t *tags; const int32_t *count; };
// the sweep plans' `totals`, behind a plan of the call's `batch` pairs (a slice's plan uses the head of the buffer, `totals` stays where it is)
int32_t *plan_totals(int32_t *plan, int batch) { return plan + 2 * (size_t)batch + 2; }
enum class Sweep { tile, split, wave }; // k_score, k_score_split, k_score_w

// The stage launchers of a chunk's sweep.  The scheduler (Pass::count ... Pass::walk, which keep the decisions, the event pairs and the launch counters) and
// the probes behind the kernel-pinning tests (mdrp_bound_models, mdrp_retire_models, mdrp_front_models, mdrp_front_lists, mdrp_replay_slots) all launch
// through here: plan kernels, grids, argument order and buffer roles are written once.  A launcher only issues launches, and records its caller's
// events, on the stream it is given.  Grids are upper bounds from the chunk's length: a workgroup beyond the plan exits at once (k_count, k_bound)
// or finds its item loop empty (the exact sweeps).

// Candidate counts on the matrix cores against the records of the chunks before this one: of (v.tags, v.model_count), survivors only go on
// (v.tags_v, v.surv1).  Phase A: every hypothesis over the pair's leading tiles (all tiles where the records, or a null cand_stat, do not allow a
// split); two_phase: phase B, the undecided ones over the rest (k_count, mdrp_kernels.h).  The undecided list lives where this chunk's SORTED list
// will be written once the counts are done (k_sort_tags), the partial counts in the other parity's sorted list, whose last reader was the previous
// chunk's exact sweep: no scratch of their own.  stats (or null): evaluations, [0] all and [1] on the matrix cores.
int launch_count(mdrp_handle *h, hipStream_t s, int kind, const ChunkView &v, bool two_phase, unsigned long long *stats, unsigned long long *cand_stat,
                 hipEvent_t c0, hipEvent_t c1) {
    uint32_t *tags_u = v.tags_sorted;
    int32_t *und_part = reinterpret_cast<int32_t *>(v.tags_sorted_other), *cplan = h->cplan.as<int32_t>();
    hipLaunchKernelGGL(k_count_plan, dim3(1), dim3(PLAN_THREADS), 0, s, v.pc, v.st, v.model_count, 2, CNT_WG_MODELS, cplan,
                       v.surv1, (const int32_t *)nullptr, two_phase ? v.und_count : (int32_t *)nullptr); // (also clears the counters k_count appends to)
    const dim3 cgrid((unsigned)v.pc * (unsigned)((v.r.chunk_len * v.r.mps + CNT_WG_MODELS - 1) / CNT_WG_MODELS));
    HIPCHK(hipEventRecord(c0, s));
    MDRP_SWEEP_DISPATCH(k_count, kind, cgrid, dim3(CNT_THREADS), 0, s, v.r, v.st, v.rfrag, v.models,
                        v.tags, v.model_count, cplan, v.tags_v, v.surv1, stats, (int32_t *)nullptr, (const int32_t *)nullptr,
                        1, tags_u, und_part, v.und_count, (const int32_t *)nullptr, cand_stat);
    if (two_phase) {
        hipLaunchKernelGGL(k_count_plan, dim3(1), dim3(PLAN_THREADS), 0, s, v.pc, v.st, v.und_count, 2, CNT_WG_MODELS, cplan,
                           (int32_t *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr);
        MDRP_SWEEP_DISPATCH(k_count, kind, cgrid, dim3(CNT_THREADS), 0, s, v.r, v.st, v.rfrag, v.models,
                            tags_u, v.und_count, cplan, v.tags_v, v.surv1, stats, (int32_t *)nullptr, (const int32_t *)nullptr,
                            2, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, und_part, cand_stat);
    }
    HIPCHK(hipEventRecord(c1, s));
    return MDRP_OK;
}

// fp32 lower bound of the score for k_count's survivors (v.tags_v, v.surv1); its survivors go back into the chunk's tag list (v.tags, v.surv2),
// which k_count has consumed, and are what `sv` names afterwards.  dbg_lb / dbg_ub (or null): the two bounds of every model (mdrp_bound_models).
int launch_bound(mdrp_handle *h, hipStream_t s, int kind, const ChunkView &v, unsigned long long *stats, double *dbg_lb, int32_t *dbg_ub,
                 hipEvent_t b0, hipEvent_t b1, Survivors &sv) {
    int32_t *cplan = h->cplan.as<int32_t>();
    hipLaunchKernelGGL(k_count_plan, dim3(1), dim3(PLAN_THREADS), 0, s, v.pc, v.st, v.surv1, 1, BND_THREADS, cplan, v.surv2, (const int32_t *)nullptr);
    const dim3 bgrid((unsigned)v.pc * (unsigned)((v.r.chunk_len * v.r.mps + BND_THREADS - 1) / BND_THREADS));
    HIPCHK(hipEventRecord(b0, s));
    MDRP_SWEEP_DISPATCH(k_bound, kind, bgrid, dim3(BND_THREADS), 0, s, v.r, v.st, v.pts, v.models, v.tags_v, v.surv1, cplan, v.tags, v.surv2, stats,
                        dbg_lb, dbg_ub);
    HIPCHK(hipEventRecord(b1, s));
    sv = Survivors{v.tags, v.surv2};
    return MDRP_OK;
}

// sort by candidate density, plan, exact fp64 sweep of the survivors between the events e0 and e1:
//   k_score_w      calls of few pairs: one WAVEFRONT per hypothesis — a lane per hypothesis is a 0.3 ms serial record loop however few there are
//   k_score_split  the survivors of k_bound (~93 per pair): 64 hypotheses per workgroup, each wavefront a quarter of the records
//   k_score        a run's first chunk: its sweep runs beside the second chunk's solver, where more and smaller sweep workgroups only wait longer
int launch_score(mdrp_handle *h, hipStream_t s, int kind, const ChunkView &v, const Survivors &sv, Sweep sweep, int32_t *plan, int32_t *totals,
                 hipEvent_t e0, hipEvent_t e1) {
    const bool wave = sweep == Sweep::wave, split = sweep == Sweep::split;
    const int models = v.r.chunk_len * v.r.mps;
    if (wave) hipLaunchKernelGGL(k_count_plan, dim3(1), dim3(PLAN_THREADS), 0, s, v.pc, v.st, sv.count, 1, SCW_THREADS / 64, plan, (int32_t *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr);
    hipLaunchKernelGGL(k_sort_tags, dim3(v.pc), dim3(256), 0, s, v.r, v.st, v.model_count, sv.count, sv.tags, v.tags_sorted);
    if (!wave) hipLaunchKernelGGL(k_plan, dim3(1), dim3(PLAN_THREADS), 0, s, v.pc, v.model_count, plan, totals, split ? SPLIT_HYP : SCORE_THREADS);
    HIPCHK(hipEventRecord(e0, s));
    const long long capped = (long long)h->num_cu * 32; // k_score_w, k_score_split: surplus workgroups exit at once, a shortfall is taken by the item loop
    if (wave) {
        const long long ub = (long long)v.pc * ((models + SCW_THREADS / 64 - 1) / (SCW_THREADS / 64));
        MDRP_SWEEP_DISPATCH(k_score_w, kind, dim3((unsigned)std::min(ub, capped)), dim3(SCW_THREADS), 0, s, v.r, v.st, v.pts, v.models, v.tags_sorted, v.model_count,
                            v.slot_score, v.slot_inl, plan);
    } else if (split) {
        const long long ub = (long long)v.pc * ((models + SPLIT_HYP - 1) / SPLIT_HYP + 1); // items: at most ceil(sparse / 64) + ceil(dense / 64) per pair
        MDRP_SWEEP_DISPATCH(k_score_split, kind, dim3((unsigned)std::min(ub, capped)), dim3(SPLIT_THREADS), 0, s, v.r, v.st, v.pts, v.models, v.tags_sorted, v.model_count,
                            v.slot_score, v.slot_inl, plan, totals);
    } else {
        const dim3 grid((unsigned)v.pc * (unsigned)((models + SCORE_THREADS - 1) / SCORE_THREADS));
        MDRP_SWEEP_DISPATCH(k_score, kind, grid, dim3(SCORE_THREADS), SCORE_TILE_BYTES, s, v.r, v.st, v.pts, v.models, v.tags_sorted, v.model_count,
                            v.slot_score, v.slot_inl, plan, totals);
    }
    HIPCHK(hipEventRecord(e1, s));
    return MDRP_OK;
}

// A run's first chunk in calls of more than SCORE_WAVE_MAX_PAIRS pairs (3-point estimators): prefix retirement (mdrp_kernels.h, "first chunk").
// In: k_count's survivors — every live hypothesis, or what a prior's records left.  The picked ones are scored here; what their prefix records
// do not retire is back on the kept list for the exact sweep.  The picked list uses the chunk's solver-order tag list (k_count has consumed it), the
// rest list the other parity's sorted list (free until the next chunk's count), their counters surv2 and und_count (idle in a first chunk).
struct FrontLists { uint32_t *pick, *rest, *kept; int32_t *n_pick, *n_rest /*stride 2*/, *n_kept; };
FrontLists front_lists(const ChunkView &v) { return FrontLists{v.tags, v.tags_sorted_other, v.tags_v, v.surv2, v.und_count, v.surv1}; }
// ... its three parts (mdrp_front_lists runs the first and the last around its caller's tables): the pick,
void launch_front_pick(hipStream_t s, const ChunkView &v, const Survivors &sv, int first_pick) {
    const FrontLists f = front_lists(v);
    hipLaunchKernelGGL(k_first_pick, dim3(v.pc), dim3(FIRST_THREADS), 0, s, v.r, v.st, sv.count, sv.tags, first_pick, f.pick, f.n_pick, f.rest, f.n_rest);
}
// the picked hypotheses' exact scores between the events f0 and f1,
int launch_front_score(mdrp_handle *h, hipStream_t s, int kind, const ChunkView &v, int32_t *plan, int32_t *totals, hipEvent_t f0, hipEvent_t f1) {
    const FrontLists f = front_lists(v);
    hipLaunchKernelGGL(k_sort_tags, dim3(v.pc), dim3(256), 0, s, v.r, v.st, v.model_count, f.n_pick, f.pick, v.tags_sorted);
    hipLaunchKernelGGL(k_plan, dim3(1), dim3(PLAN_THREADS), 0, s, v.pc, v.model_count, plan, totals, SPLIT_HYP);
    HIPCHK(hipEventRecord(f0, s));
    const long long ub = 2ll * v.pc; // at most FIRST_PICK_MAX + 1 hypotheses per pair, in two density classes: two workgroups of SPLIT_HYP
    MDRP_SWEEP_DISPATCH(k_first_score, kind, dim3((unsigned)std::min(ub, (long long)h->num_cu * 32)), dim3(SPLIT_THREADS), 0, s, v.r, v.st, v.pts, v.models,
                        v.tags_sorted, v.model_count, v.slot_score, v.slot_inl, plan, totals);
    HIPCHK(hipEventRecord(f1, s));
    return MDRP_OK;
}
// and the filter of the rest list by their records (evals: the counter k_first_filter adds to), whose kept list is what goes on to the exact sweep.
Survivors launch_front_filter(hipStream_t s, const ChunkView &v, unsigned long long *evals) {
    const FrontLists f = front_lists(v);
    hipLaunchKernelGGL(k_first_filter, dim3(v.pc), dim3(FIRST_THREADS), 0, s, v.r, v.st, v.slot_score, v.slot_inl, f.pick, f.n_pick, f.rest, f.n_rest,
                       f.kept, f.n_kept, evals);
    return Survivors{f.kept, f.n_kept};
}
// The scheduler (Pass::front) and mdrp_front_models run the three in a row.
int launch_front(mdrp_handle *h, hipStream_t s, int kind, const ChunkView &v, int first_pick, int32_t *plan, int32_t *totals, unsigned long long *evals,
                 hipEvent_t f0, hipEvent_t f1, Survivors &sv) {
    launch_front_pick(s, v, sv, first_pick);
    if (int rc = launch_front_score(h, s, kind, v, plan, totals, f0, f1)) return rc;
    sv = launch_front_filter(s, v, evals);
    return MDRP_OK;
}

// Replay of score_models / ransac bookkeeping over the ordered triggers of `batch` pairs; with budgets (n_bud of them, else null), the walk that
// takes their checkpoints into ckpt.
void launch_walk(hipStream_t s, int batch, const RunParams &r, PairState *st, const Model *models, const Trigger *trig, int trig_cap, Progress *progress,
                 const uint64_t *budgets, int n_bud, PairState *ckpt) {
    if (budgets)
        hipLaunchKernelGGL(k_walk_ckpt, dim3((batch + WALK_CKPT_THREADS - 1) / WALK_CKPT_THREADS), dim3(WALK_CKPT_THREADS), 0, s, r, st, models, trig, trig_cap,
                           &progress->n_active, &progress->max_needed, budgets, n_bud, ckpt);
    else
        hipLaunchKernelGGL(k_walk, dim3((batch + 63) / 64), dim3(64), 0, s, r, st, models, trig, trig_cap, &progress->n_active, &progress->max_needed,
                           (const int32_t *)nullptr, 0, 0, 0);
}

// A pass and the stages run_pass strings together.  Stages only issue work (launches, copies, memsets, events) on the stream they name; who waits for
// whom is run_pass's business.
struct Pass : PassIn {
    mdrp_handle *const h;
    const hipStream_t s; // the main stream
    const int est_shift;
    const bool classic; // non-monodepth baselines (mdrp_classic.h)
    const int mps, ssz;
    // Run-time knobs (DESIGN.md 10 lists all of them; defaults that depend on the call's shape: mdrp_schedule.h)
    const bool lo_overlap = env_int("MDRP_LO_OVERLAP", 1) != 0;     // three-stream pipeline; 0 = every kernel on the handle's stream
    const bool use_bound = env_int("MDRP_BOUND", 1) != 0;           // fp32 lower-bound stage between k_count and the fp64 sweep
    const bool score_split = env_int("MDRP_SCORE_SPLIT", 1) != 0;   // exact sweeps after a run's first chunk: k_score_split; 0 = k_score
    // a run's first chunk: hypotheses scored first, whose prefix records retire most of the others (k_first_*); 0 = the whole chunk is scored as before
    const int first_pick = sched::first_pick(kind, batch_call, SCORE_WAVE_MAX_PAIRS, env_int("MDRP_FIRST_PICK", -1));
    // solver wavefronts per SIMD beside a first chunk's sweeps (sched::solver_reservation); set: that R with no LDS kept free, 0 = uncapped
    const int solve_resident = env_int("MDRP_SOLVE_RESIDENT", -1);
    // a run's second chunk: its solver starts behind k_prep (sched::second_solver_after); 0 = behind the first chunk's solver
    const int solve_behind_prep = env_int("MDRP_SOLVE_BEHIND_PREP", -1);
    // the first super-chunk's small blocks are cleared by one kernel in front of k_prep (clear_front); 0 = one memset each where they are used
    const bool front_clear = front_clear_on();
    // the scan behind a chunk with a bar reads the exact sweep's lists (k_scan_list); 0 = it walks every slot.  The cap: candidates per pair the list
    // scan takes (pairs with more are walked in full; the tests lower it to reach that path)
    const bool scan_list = env_int("MDRP_SCAN_LIST", 1) != 0;
    const int scan_list_cap = env_int("MDRP_SCAN_LIST_CAP", SCAN_LIST_MAX);
    const int lo_threads = env_int("MDRP_LO_THREADS", sched::lo_lanes(batch_call, n_max));
    const int final_threads = env_int("MDRP_FINAL_THREADS", sched::final_lanes(batch_call));
    const int samp_threads = env_int("MDRP_SAMPLE_THREADS", ssz == 3 ? SAMP_THREADS : (ssz == 5 ? 512 : 256)); // ~ samples between two rejections
    const int lo_blocks = h->num_cu * (lo_threads == 64 ? 8 : 2);
    // the inlier-only final refinement walks a compacted index of the inliers instead of masking every record (where the three lists fit 32 KiB of LDS)
    const int mask_index = lm_mask_index_on(n_max);
    // work lists of the classic LM (mdrp_classic.h ClmList)
    const int clm_list_stride = lm_list_stride(n_max);
    const size_t clm_list_bytes = (size_t)2 * clm_list_stride * sizeof(uint16_t);
    // Fused tail (mdrp_kernels.h FuseTail): when the end of the run is known on the host (the super-chunk reaches max_iterations), the
    // last LO launch replays each pair as its last trigger is refined (no k_walk launch), and k_final starts - on the main stream,
    // behind k_gate - as soon as the LO queue is empty, taking pairs in the order they became ready: the final refinements fill
    // the wavefront slots the LO's stragglers leave free, instead of LO | k_walk | k_final one after the other.
    // Measured per 1024 pairs (N = 2000, 10^4 iterations): calibrated 11.75 -> 11.2 ms, shared focal 12.5 -> 11.9, outlier-free 18.6 -> 17.4;
    // with the shift solver's 9-parameter LM the final refinements are 1.5x the LO's tail and gain nothing (12.75 -> 12.9 ms): off there.
    // After a bounded wait expired on this handle (kernels of two streams do not run side by side here: serialising profiler,
    // AMD_SERIALIZE_KERNEL, a busy shared GPU) the handle stays unfused, unless MDRP_FUSE_TAIL is set explicitly.
    // (fuse_disabled / fuse_retry_in are advanced once per API call in estimate_device, not per pass)
    // (a budgets call runs its tail unfused: the checkpoints are taken by the walk kernel, and their refinements are one launch of their own)
    const bool fuse_env = !bud && env_int("MDRP_FUSE_TAIL", ((kind == MDRP_CALIB && est_shift) || h->fuse_disabled) ? 0 : 1) != 0;
    const int n_bud = bud ? bud->n : 0;
    const int trig_cap = chunk_cap;
    const size_t groups_max = ((size_t)n_max + 15) / 16;

    std::vector<int32_t> table_of, tab_n;
    int n_tables = 0;
    uint64_t certain = 0;
    sched::Lead lead;
    PassScratch sz;
    RunParams rp;
    // the `params` block on the device, and the counter block
    unsigned char *pd = nullptr;
    uint64_t *d_table_state = nullptr;
    CamDev *d_cams1 = nullptr, *d_cams2 = nullptr;
    int32_t *d_table_n = nullptr, *d_table_of = nullptr, *d_nper = nullptr;
    Counters *cnt = nullptr;
    // the super-chunk under way
    uint64_t it0 = 0;
    sched::Layout lay;
    bool piped = false, fuse_tail = false, presampled[2] = {false, false};
    bool front_cleared = false, fuse_cleared = false; // clear_front has filled the first super-chunk's blocks (and the fused tail's)
    hipStream_t aux = nullptr, aux2 = nullptr; // the handle's, or `s` where the super-chunk is not pipelined
    int32_t *fz_ctl = nullptr, *fz_done = nullptr, *fz_fin = nullptr, *fz_ready = nullptr;
    bool final_done = false; // the fused tail has run the final refinements
    ProsacTab ptab{nullptr, nullptr, nullptr}; // ranked call: the progressive sampler's tables

    Pass(mdrp_handle *h_, const PassIn &in)
        : PassIn(in), h(h_), s(h_->stream), est_shift((kind == MDRP_CALIB && ro->monodepth_estimate_shift) ? 1 : 0), classic(kind >= MDRP_RELPOSE_5PT),
          mps(sched::model_slots(kind)), ssz(sched::sample_size(kind)) {}

    // sample tables, leading chunks and scratch of the pass
    int plan_and_allocate() {
        plan();
        return allocate();
    }
    // ... the decisions alone: nothing is allocated or issued (mdrp_front_stages refuses a chunk list against them before any device work)
    void plan() {
        sched::group_tables(n_host, batch, table_of, tab_n);
        n_tables = (int)tab_n.size();
        certain = sched::certain_iterations(ro->max_iterations, ro->min_iterations);
        const bool chunks_set = sched::parse_chunks(getenv("MDRP_CHUNKS"), lead);
        if (h->wish_kind >= 0 && hipEventQuery(h->ev_wish) == hipSuccess) { // an unfused run's sums have arrived
            if (h->wish_host[1] > 0) h->seen_wish[h->wish_kind] = (double)h->wish_host[0] / (double)h->wish_host[1];
            h->wish_kind = -1;
        }
        if (!chunks_set) lead = sched::default_lead(kind, certain, kind <= MDRP_VARYING_FOCAL ? h->seen_wish[kind] : -1.0);
        sz = pass_scratch(h, kind, batch, n_max, n_tables, chunk_cap, lead.first(), n_bud);
    }
    int allocate() {
        for (const auto &b : sz.bufs) {
            if (int rc = b.first->ensure(b.second)) return rc; // (0 bytes: nothing to allocate)
            // the small per-call inputs travel as one block (six pageable copies cost ~60 us of an idle GPU in front of k_prep)
            if (b.first == &h->params && h->params_host_cap < sz.params) {
                h->params_host.reset(); h->params_host_cap = 0;
                HIPCHK(hipHostMalloc((void **)&h->params_host.v, sz.params + sz.params / 2, hipHostMallocDefault));
                h->params_host_cap = sz.params + sz.params / 2;
            }
        }
        pd = h->params.as<unsigned char>();
        d_table_state = reinterpret_cast<uint64_t *>(pd);
        d_cams1 = reinterpret_cast<CamDev *>(pd + sz.off_cam1); d_cams2 = reinterpret_cast<CamDev *>(pd + sz.off_cam2);
        d_table_n = reinterpret_cast<int32_t *>(pd + sz.off_tn); d_table_of = reinterpret_cast<int32_t *>(pd + sz.off_tof);
        d_nper = reinterpret_cast<int32_t *>(pd + sz.off_nper);
        cnt = h->counters.as<Counters>();
        return MDRP_OK;
    }

    // the per-call parameters in one H2D copy on the main stream, and the run parameters every kernel takes by value
    int upload_params() {
        unsigned char *ph = h->params_host; // free: the previous call on this handle ended with a stream synchronisation
        const std::vector<uint64_t> tab_state(n_tables, ro->seed);
        std::memcpy(ph, tab_state.data(), sizeof(uint64_t) * n_tables);
        const bool cams = kind == MDRP_CALIB || kind == MDRP_RELPOSE_5PT || kind == MDRP_SHARED_6PT;
        // MDRP_SHARED_6PT reads the principal point from cam1 only (include/mdrp.h): cam2 may be NULL there
        if (cams) { std::memcpy(ph + sz.off_cam1, cam1, sizeof(CamDev) * batch); std::memcpy(ph + sz.off_cam2, cam2 ? cam2 : cam1, sizeof(CamDev) * batch); }
        else std::memset(ph + sz.off_cam1, 0, 2 * sizeof(CamDev) * (size_t)batch);
        std::memcpy(ph + sz.off_tn, tab_n.data(), sizeof(int32_t) * n_tables);
        std::memcpy(ph + sz.off_tof, table_of.data(), sizeof(int32_t) * batch);
        std::memcpy(ph + sz.off_nper, n_host, sizeof(int32_t) * batch);
        if (bud) std::memcpy(ph + sz.off_bud, bud->budgets, sizeof(uint64_t) * n_bud);
        HIPCHK(hipMemcpyAsync(pd, ph, sz.params, hipMemcpyHostToDevice, s));
        if (prosac) { if (int rc = prosac_tables(h, s, ssz, tab_n.data(), n_tables, *prosac, ro->max_iterations, ptab)) return rc; }

        std::memset(&rp, 0, sizeof rp);
        rp.kind = kind; rp.solver = solver_for(kind, est_shift); rp.est_shift = est_shift;
        rp.score_initial = ro->score_initial_model ? 1 : 0;
        rp.batch = batch; rp.n_max = n_max;
        rp.max_iterations = ro->max_iterations; rp.min_iterations = ro->min_iterations;
        rp.dyn_mult = ro->dyn_num_trials_mult; rp.log_prob_missing = std::log(1.0 - ro->success_prob);
        rp.weight_sampson = ro->monodepth_weight_sampson > 0.0f ? (double)ro->monodepth_weight_sampson : 0.0; // the wrappers hand max(ws, 0) on (@0x2246e6)
        rp.final_max_it = (int)std::min<uint64_t>(bo->max_iterations, 1u << 30); rp.final_loss = bo->loss_type;
        rp.grad_tol = bo->gradient_tol; rp.step_tol = bo->step_tol; rp.lambda0 = bo->initial_lambda;
        rp.lambda_min = bo->min_lambda; rp.lambda_max = bo->max_lambda;
        rp.chunk_len = chunk_cap; rp.chunk_off = 0; rp.slot_stride = chunk_cap * mps; rp.super_len = chunk_cap; rp.chunk_start = 0;
        rp.mps = mps; rp.sample_sz = ssz;
        return MDRP_OK;
    }

    // Device-resident inputs: what the run's first super-chunk starts from, filled by ONE kernel on the main stream in front of the parameter upload
    // and k_prep, where the GPU has nothing else to do — the counters, the candidate statistics, the model counts of both chunk parities, the fused
    // tail's block where that super-chunk will end with the fused tail, and (the call's first pass) the LM statistics.  begin_super_chunk, solve and
    // lo then issue no memset for it; later super-chunks, the sliced host front and the stage-by-stage entry points keep theirs.
    // Stream order covers every block: each is last read by the previous pass or call on the main stream or behind an event the main stream has
    // waited for (the LO launch on aux2: ev_lo; the solvers on aux: ev_solved), and first written behind an event recorded on the main stream after
    // this launch (the second chunk's solver on aux: ev_prepped or ev_solved[0]; the LO launch on aux2: ev_scanned).  The ready list of the fused tail
    // (all ones) is read by the previous k_final on the main stream and published to by this pass's k_lo behind ev_scanned.
    int clear_front() {
        if (!front_clear || host) return MDRP_OK;
        const sched::Layout l0 = sched::super_chunk_layout(0, certain, chunk_cap, lead, 0, ro->max_iterations);
        const bool fuse0 = fuse_env && l0.n_chunks > 1 && lo_overlap && l0.super_len >= ro->max_iterations; // (begin_super_chunk's fuse_tail at it0 = 0)
        ClearList cl{};
        auto add = [&cl](void *p_, size_t bytes, uint32_t value) {
            cl.p[cl.n] = static_cast<uint32_t *>(p_); cl.words[cl.n] = (uint32_t)(bytes / sizeof(uint32_t)); cl.value[cl.n] = value; cl.n++;
        };
        const size_t b = (size_t)batch;
        add(h->counters.p, sizeof(Counters), 0);
        add(h->cand_stat.p, sizeof(unsigned long long) * 2 * b, 0);
        add(h->model_count[0].p, sizeof(int32_t) * 2 * b, 0);
        add(h->model_count[1].p, sizeof(int32_t) * 2 * b, 0);
        if (fuse0) {
            if (int rc = h->fuse.ensure(sz.fuse)) return rc;
            int32_t *ctl = h->fuse.as<int32_t>();
            add(ctl, 64 + 2 * sizeof(int32_t) * b, 0);              // control words | done flags | final-refinement flags
            add(ctl + 16 + 2 * b, sizeof(int32_t) * b, 0xFFFFFFFFu); // ready list
        }
        if (clear_lm_stats) add(h->lm_stats.p, LM_STATS_BYTES, 0);
        static_assert(7 <= CLEAR_BLOCKS_MAX && sizeof(Counters) % 4 == 0 && LM_STATS_BYTES % 4 == 0, "clear list");
        const int blocks = (int)std::min<size_t>(64, (4 * b + CLEAR_THREADS - 1) / CLEAR_THREADS);
        hipLaunchKernelGGL(k_clear, dim3(std::max(blocks, 1)), dim3(CLEAR_THREADS), 0, s, cl);
        front_cleared = true; fuse_cleared = fuse0;
        return MDRP_OK;
    }

    // normalisation, record layout, MFMA fragments and pair states of the pairs [p0, p0 + pc) (one workgroup per pair, bases offset by p0)
    void prep(int p0, int pc, hipStream_t st_) {
        const size_t o2 = (size_t)2 * p0 * n_max, o1 = (size_t)p0 * n_max;
        double *pts_p = h->pts.as<double>() + o1 * PT_STRIDE;
        uint4 *rfrag_p = h->rfrag.as<uint4>() + (size_t)p0 * groups_max * 64;
        if (classic)
            hipLaunchKernelGGL(kc_prep, dim3(pc), dim3(256), 0, st_, rp, x1 + o2, x2 + o2, d_nper + p0, d_table_of + p0, d_cams1 + p0, d_cams2 + p0,
                               ro->max_epipolar_error, bo->loss_scale, pts_p, h->st.as<PairState>() + p0, rfrag_p);
        else
            hipLaunchKernelGGL(k_prep, dim3(pc), dim3(256), 0, st_, rp, x1 + o2, x2 + o2, d1 + o1, d2 + o1, d_nper + p0, d_table_of + p0, d_cams1 + p0, d_cams2 + p0,
                               ro->max_epipolar_error, ro->max_reproj_error, bo->loss_scale, pts_p, h->dep.as<double>() + 2 * o1, h->st.as<PairState>() + p0, rfrag_p);
    }

    // a call with priors: every pair that has one starts from the state ransac<> is in after scoring and LO-refining it (k_prior, mdrp_prior.h).
    // On the main stream behind k_prep: every reader of the pair states is ordered behind this stream's first solver launch.
    void prior() {
        if (classic) { // kc_prior (mdrp_classic_models.h); the pass's output mask is clm_lo's subset mask: kc_final rewrites every byte of it
#define MDRP_KC_PRIOR_LAUNCH(CK)                                                                                                          \
    hipLaunchKernelGGL((kc_prior<CK>), dim3(batch), dim3(CLASSIC_MODEL_THREADS), clm_list_bytes, s, rp, h->st.as<PairState>(),            \
                       (const double *)h->pts.as<double>(), priors, prior_space, mask_dev, clm_list_stride)
            if (kind == MDRP_RELPOSE_5PT) MDRP_KC_PRIOR_LAUNCH(CLASSIC_RELPOSE);
            else if (kind == MDRP_SHARED_6PT) MDRP_KC_PRIOR_LAUNCH(CLASSIC_SHARED);
            else MDRP_KC_PRIOR_LAUNCH(CLASSIC_FUND);
#undef MDRP_KC_PRIOR_LAUNCH
            return;
        }
#define MDRP_PRIOR_LAUNCH(K, S)                                                                                                                  \
    hipLaunchKernelGGL((k_prior<K, S>), dim3(batch), dim3(PRIOR_THREADS), lm_list_bytes(n_max), s, rp, h->st.as<PairState>(),                     \
                       (const double *)h->pts.as<double>(), (const double *)h->dep.as<double>(), priors, lm_list_stride(n_max),                  \
                       h->lm_stats.as<unsigned long long>())
        if (kind == MDRP_CALIB && est_shift) MDRP_PRIOR_LAUNCH(0, true);
        else if (kind == MDRP_CALIB) MDRP_PRIOR_LAUNCH(0, false);
        else if (kind == MDRP_SHARED_FOCAL) MDRP_PRIOR_LAUNCH(1, false);
        else MDRP_PRIOR_LAUNCH(2, false);
#undef MDRP_PRIOR_LAUNCH
    }

    // the chunks of the super-chunk at it0, its cleared counters, and whether it is pipelined over the streams and ends with the fused tail
    int begin_super_chunk(uint64_t max_needed) {
        return begin_super_chunk(sched::super_chunk_layout(it0, certain, chunk_cap, lead, max_needed, ro->max_iterations));
    }
    // ... with the chunks given (mdrp_front_stages: a caller's chunk list)
    int begin_super_chunk(const sched::Layout &layout) {
        lay = layout;
        if (it0 == 0) h->first_chunk = (int64_t)lay.lens[0];
        rp.chunk_start = it0; rp.super_len = (int)lay.super_len;
        if (!(front_cleared && it0 == 0)) { // (clear_front has done both)
            HIPCHK(hipMemsetAsync(h->counters.p, 0, sizeof(Counters), s));
            if (it0 == 0) HIPCHK(hipMemsetAsync(h->cand_stat.p, 0, sizeof(unsigned long long) * 2 * batch, s));
        }
        piped = lay.n_chunks > 1 && lo_overlap;
        fuse_tail = fuse_env && piped && it0 + lay.super_len >= ro->max_iterations;
        if (fuse_tail) {
            if (int rc = h->fuse.ensure(sz.fuse)) return rc;
            fz_ctl = h->fuse.as<int32_t>(); fz_done = fz_ctl + 16; fz_fin = fz_done + batch; fz_ready = fz_fin + batch;
        }
        aux = piped ? h->aux_stream : s; aux2 = piped ? h->aux_stream2 : s;
        presampled[0] = presampled[1] = false;
        return MDRP_OK;
    }

    void samples(hipStream_t st_, int len_, uint32_t *smp_) {
        if (prosac) launch_samples_prosac(st_, ssz, samp_threads, n_tables, d_table_n, d_table_state, ptab, *prosac, len_, smp_);
        else if (ssz == 6) hipLaunchKernelGGL(kc_samples<6>, dim3(n_tables), dim3(samp_threads), 0, st_, n_tables, d_table_n, d_table_state, len_, smp_);
        else if (ssz == 5) hipLaunchKernelGGL(kc_samples<5>, dim3(n_tables), dim3(samp_threads), 0, st_, n_tables, d_table_n, d_table_state, len_, smp_);
        else if (ssz == 7) hipLaunchKernelGGL(kc_samples<7>, dim3(n_tables), dim3(samp_threads), 0, st_, n_tables, d_table_n, d_table_state, len_, smp_);
        else hipLaunchKernelGGL(k_samples, dim3(n_tables), dim3(samp_threads), 0, st_, n_tables, d_table_n, d_table_state, len_, smp_);
    }
    // The sample tables of a run's first two chunks do not depend on anything but (seed, N): they are drawn on the (still idle)
    // LO stream while k_prep runs, so the one-workgroup-per-table sampler (0.18 ms for 10^4 samples) is off the solver's path.
    int presample() {
        HIPCHK(hipStreamWaitEvent(aux2, h->ev_tables, 0));
        for (int c = 0; c < 2 && c < lay.n_chunks; ++c) {
            samples(aux2, (int)lay.lens[c], h->samples[c & 1].as<uint32_t>());
            HIPCHK(hipEventRecord(h->ev_sampled[c], aux2));
            presampled[c] = true;
        }
        return MDRP_OK;
    }

    ChunkView view(int c, int p0, int pc) const {
        ChunkView v;
        const bool odd = c & 1;
        const size_t so = (size_t)p0 * rp.slot_stride, o1 = (size_t)p0 * n_max, q = (size_t)p0;
        v.c = c; v.p0 = p0; v.pc = pc; v.first_of_run = it0 == 0 && c == 0;
        v.r = rp; v.r.chunk_len = (int)lay.lens[c]; v.r.chunk_off = lay.offs[c]; v.r.batch = pc;
        v.st = h->st.as<PairState>() + q; v.pts = h->pts.as<double>() + o1 * PT_STRIDE; v.dep = classic ? nullptr : h->dep.as<double>() + o1 * 2;
        v.models = h->models.as<Model>() + so; v.slot_score = h->slot_score.as<double>() + so; v.slot_inl = h->slot_inl.as<int32_t>() + so;
        v.samples = h->samples[odd].as<uint32_t>(); v.tags = h->tags[odd].as<uint32_t>() + so; v.tags_v = h->tags_v.as<uint32_t>() + so;
        v.tags_sorted = h->tags_sorted[odd].as<uint32_t>() + so; v.tags_sorted_other = h->tags_sorted[!odd].as<uint32_t>() + so;
        v.model_count = h->model_count[odd].as<int32_t>() + 2 * q; v.und_count = h->und_count.as<int32_t>() + 2 * q;
        v.surv1 = h->surv_count.as<int32_t>() + q; v.surv2 = h->surv2_count.as<int32_t>() + q;
        v.cand_stat = h->cand_stat.as<unsigned long long>() + 2 * q;
        v.rfrag = h->rfrag.as<uint4>() + q * groups_max * 64; v.trig = h->triggers.as<Trigger>() + q * trig_cap;
        return v;
    }

    // Dynamic LDS each solver workgroup of the view reserves (and never touches), or 0: no cap.  Only the long solver that shares the chip with a
    // first chunk's prefix retirement (P3P and shift solvers: the focal ones sit at two wavefronts per SIMD by their registers) is ever capped.
    // Unset, MDRP_SOLVE_RESIDENT means sched::SOLVE_RESIDENT with two of the front's largest sweep workgroups kept free.
    size_t solve_reserve(const ChunkView &v) const {
        const bool beside_front = piped && it0 == 0 && v.c == 1 && kind == MDRP_CALIB;
        if (!beside_front || solve_resident == 0 || (solve_resident < 0 && first_pick == 0)) return 0;
        const size_t sweep_wg = std::max<size_t>(SPLIT_LDS_BYTES, std::max<size_t>(SCORE_TILE_BYTES, CNT_LDS_BYTES));
        return solve_resident > 0 ? sched::solver_reservation(h->lds_per_cu, solve_resident, 0)
                                  : sched::solver_reservation(h->lds_per_cu, sched::SOLVE_RESIDENT, 2 * sweep_wg);
    }

    // sample table (unless presampled) and minimal solver of the view on stream st_
    int solve(const ChunkView &v, hipStream_t st_) {
        const RunParams &r = v.r;
        const int pc = v.pc;
        // (clear_front has cleared both parities for the first two chunks of the run; a third chunk takes the first one's over)
        if (!(front_cleared && it0 == 0 && v.c < 2)) HIPCHK(hipMemsetAsync(v.model_count, 0, sizeof(int32_t) * 2 * pc, st_));
        if (v.c < 2 && presampled[v.c]) HIPCHK(hipStreamWaitEvent(st_, h->ev_sampled[v.c], 0));
        else samples(st_, r.chunk_len, v.samples);
        hipEvent_t v0, v1;
        if (int rc = get_events(h, &v0, &v1, 5)) return rc;
        HIPCHK(hipEventRecord(v0, st_));
        struct Stop { hipEvent_t e; hipStream_t s; ~Stop() { (void)hipEventRecord(e, s); } } stop_{v1, st_}; // after the solver launch below
        if (classic) {
            const dim3 sgrid((r.chunk_len + 63) / 64, pc);
            if (kind == MDRP_SHARED_6PT)
                hipLaunchKernelGGL(kc_solve<CLASSIC_SHARED>, sgrid, dim3(64), 0, st_, r, v.st, v.samples, v.pts, v.models, v.slot_inl, v.tags, v.model_count);
            else if (kind == MDRP_RELPOSE_5PT) {
                // three kernels (mdrp_classic.h): null space and roots + poses at six wavefronts per CU, the elimination between them at three
                // Invariant: two solves that may run at the same time never share a Reduce5 block.  A chunk's solve writes blocks
                // [p0 * sgrid.x, (p0 + pc) * sgrid.x) of its region, and only the first chunk of a super-chunk of several chunks is ever solved
                // beside another chunk's solver (the sliced front: chunk 0 on `s`, chunk 1 on `aux`): it alone uses the second region.  Every
                // other solve is ordered behind the previous one by its stream or by ev_solved.
                const bool first_region = v.c == 0 && lay.n_chunks > 1;
                if (first_region && (size_t)sgrid.x > sz.red5_first_blocks) { g_err = "5-point first chunk longer than its Reduce5 region"; return MDRP_ERR_INVALID; }
                double *red5 = h->red5.as<double>() + ((first_region ? (size_t)batch * sz.red5_blocks : 0) + (size_t)v.p0 * sgrid.x) * RED5_STRIDE * 64;
                hipLaunchKernelGGL(kc_solve5_null, sgrid, dim3(64), SOLVE5N_LDS_BYTES, st_, r, v.st, v.samples, v.pts, red5);
                hipLaunchKernelGGL(kc_solve5_reduce, sgrid, dim3(64), SOLVE5_LDS_BYTES, st_, r, v.st, red5);
                hipLaunchKernelGGL(kc_solve5_roots, sgrid, dim3(64), SOLVE5B_LDS_BYTES, st_, r, v.st, v.samples, v.pts, red5, v.models, v.slot_inl, v.tags, v.model_count);
            }
            else
                hipLaunchKernelGGL(kc_solve<CLASSIC_FUND>, sgrid, dim3(64), SOLVE7_LDS_BYTES, st_, r, v.st, v.samples, v.pts, v.models, v.slot_inl, v.tags, v.model_count);
            return MDRP_OK;
        }
        // One-wavefront workgroups at a capped residency for the solver that runs beside a first chunk's sweeps, where the rule grants a cap
        // (solve_reserve); four-wavefront workgroups for the calibrated solvers otherwise (solve_threads, mdrp_kernels.h)
        const size_t reserve = solve_reserve(v);
#define MDRP_SOLVE_LAUNCH(S)                                                                                                   \
    do {                                                                                                                       \
        const int threads_ = reserve ? 64 : solve_threads(S);                                                                  \
        hipLaunchKernelGGL(k_solve<S>, dim3((r.chunk_len + threads_ - 1) / threads_, pc), dim3(threads_), reserve, st_, r, v.st, v.samples, v.pts, v.dep, v.models, v.slot_inl, v.tags, v.model_count, 0, r.chunk_len); \
    } while (0)
        switch (r.solver) {
        case SOLVER_P3P: MDRP_SOLVE_LAUNCH(SOLVER_P3P); break;
        case SOLVER_SHIFT: MDRP_SOLVE_LAUNCH(SOLVER_SHIFT); break;
        case SOLVER_SHARED: MDRP_SOLVE_LAUNCH(SOLVER_SHARED); break;
        default: MDRP_SOLVE_LAUNCH(SOLVER_VARYING); break;
        }
#undef MDRP_SOLVE_LAUNCH
        return MDRP_OK;
    }

    // The sweep stages: each decides whether and how its stage runs and keeps the call's accounting (the event pair and its `what` code, the launch
    // counters); the launches themselves are the launchers' above.
    // A run's first chunk has no record: phase A is the whole count, no phase B.
    int count(const ChunkView &v) {
        hipEvent_t c0, c1;
        if (int rc = get_events(h, &c0, &c1, 1)) return rc;
        const bool two_phase = !v.first_of_run;
        h->count_launches += two_phase ? 2 : 1; // (mdrp_stats::count_launches counts kernel launches: a rocprof summary shows the same number)
        return launch_count(h, s, kind, v, two_phase, &cnt->progress.evals, v.cand_stat, c0, c1);
    }

    // (calls of a few pairs skip the bound: its lane-per-hypothesis record loop is 0.1 ms of latency, and k_score_w takes k_count's survivors at once;
    // a run's first chunk has no records yet: nothing to retire)
    int bound(const ChunkView &v, Survivors &sv) {
        sv = Survivors{v.tags_v, v.surv1};
        if (!(use_bound && batch_call > 16 && !v.first_of_run)) return MDRP_OK;
        hipEvent_t b0, b1;
        if (int rc = get_events(h, &b0, &b1, 4)) return rc;
        return launch_bound(h, s, kind, v, &cnt->progress.evals_bound, nullptr, nullptr, b0, b1, sv);
    }

    // A run's first chunk in calls of more than SCORE_WAVE_MAX_PAIRS pairs (3-point estimators): prefix retirement
    int front(const ChunkView &v, Survivors &sv) {
        if (!(v.first_of_run && first_pick > 0)) return MDRP_OK;
        int32_t *plan = h->plan.as<int32_t>();
        hipEvent_t f0, f1;
        if (int rc = get_events(h, &f0, &f1, 0)) return rc;
        h->sweep_launches++;
        return launch_front(h, s, kind, v, first_pick, plan, plan_totals(plan, batch), &cnt->progress.evals_sweep, f0, f1, sv);
    }

    // the exact sweep between the events e0 and e1: by wavefronts in calls of few pairs, else split behind k_bound, by tiles in a run's first chunk
    int score(const ChunkView &v, const Survivors &sv, hipEvent_t e0, hipEvent_t e1) {
        const Sweep sweep = batch_call <= SCORE_WAVE_MAX_PAIRS ? Sweep::wave : (score_split && !v.first_of_run ? Sweep::split : Sweep::tile);
        int32_t *plan = h->plan.as<int32_t>();
        h->sweep_launches++;
        return launch_score(h, s, kind, v, sv, sweep, plan, plan_totals(plan, batch), e0, e1);
    }


    // ordered prefix over the iterations: LO triggers
    void scan(const ChunkView &v) {
        if (scan_list && !v.first_of_run) // (a first chunk's NaN-model slots are on no list, and most of its slots hold a result)
            launch_scan_list(s, mps, v.pc, v.r, v.st, v.slot_score, v.slot_inl, v.trig, trig_cap, v.model_count, v.tags_sorted, scan_list_cap,
                             &cnt->progress.evals_sweep);
        else (void)launch_scan(s, mps, v.pc, v.r, v.st, v.slot_score, v.slot_inl, v.trig, trig_cap, v.model_count, &cnt->progress.evals_sweep);
    }

    // count -> bound -> sort -> plan -> exact score -> scan of the view, on the main stream
    int sweep(const ChunkView &v) {
        hipEvent_t e0, e1;
        Survivors sv;
        int rc;
        if ((rc = get_events(h, &e0, &e1, 0)) || (rc = count(v)) || (rc = bound(v, sv)) || (rc = front(v, sv)) || (rc = score(v, sv, e0, e1))) return rc;
        scan(v);
        return MDRP_OK;
    }

    // The first chunk of pairs [q0, q0 + qc) of the sliced front.  The 6-point solver (11.5 KB of scratch per lane) solves it on the solver stream
    // too, behind the second chunk's slices: two of its dispatches at once on two queues need two whole-device scratch areas (~6 GB each) at the same
    // time, and the runtime aborts the queue (out of resources) when it cannot have the second one.  The main stream sweeps behind that solve.
    int first_chunk_of(int q0, int qc) {
        const ChunkView v = view(0, q0, qc);
        int rc;
        if (kind != MDRP_SHARED_6PT) { if ((rc = solve(v, s))) return rc; }
        else {
            if ((rc = solve(v, aux))) return rc;
            HIPCHK(hipEventRecord(h->ev_solved6, aux));
            HIPCHK(hipStreamWaitEvent(s, h->ev_solved6, 0));
        }
        return sweep(v);
    }
    // Host buffers (MDRP_MEM_HOST) of a run's first super-chunk: the correspondences arrive slice by slice on the copy stream; k_prep and the second
    // chunk's solver (the long one: 1.6 ms per 1024 pairs) of slice i run while slice i + 1 is on its way over PCIe.
    // solved1: the second chunk's solver has been issued; swept0: pairs whose first chunk has been swept already.
    int host_front(bool &solved1, int &swept0) {
        int rc;
        const bool sliced = piped && lay.n_chunks >= 2 && batch >= 2 * HOST_SLICE_PAIRS;
        const int sl = sliced ? HOST_SLICE_PAIRS : batch;
        for (int p0 = 0; p0 < batch; p0 += sl) {
            const int pc = std::min(sl, batch - p0);
            const size_t o2 = (size_t)2 * p0 * n_max, o1 = (size_t)p0 * n_max, n2 = sizeof(double) * 2 * (size_t)pc * n_max, n1 = sizeof(double) * (size_t)pc * n_max;
            hipStream_t cs = sliced ? h->copy_stream : s;
            HIPCHK(hipMemcpyAsync(const_cast<double *>(x1) + o2, host->x1 + o2, n2, hipMemcpyHostToDevice, cs));
            HIPCHK(hipMemcpyAsync(const_cast<double *>(x2) + o2, host->x2 + o2, n2, hipMemcpyHostToDevice, cs));
            if (host->d1 && host->d2) {
                HIPCHK(hipMemcpyAsync(const_cast<double *>(d1) + o1, host->d1 + o1, n1, hipMemcpyHostToDevice, cs));
                HIPCHK(hipMemcpyAsync(const_cast<double *>(d2) + o1, host->d2 + o1, n1, hipMemcpyHostToDevice, cs));
            }
            if (!sliced) { prep(p0, pc, s); break; }
            // k_prep and the long solver of the slice on the solver stream, beside the next slices' copies (the main stream sweeps the first chunk)
            HIPCHK(hipEventRecord(h->ev_copied, cs)); HIPCHK(hipStreamWaitEvent(aux, h->ev_copied, 0));
            if (p0 == 0) HIPCHK(hipStreamWaitEvent(aux, h->ev_tables, 0)); // (the per-call parameters were uploaded on the main stream)
            prep(p0, pc, aux);
            HIPCHK(hipEventRecord(h->ev_prepped, aux));
            if ((rc = solve(view(1, p0, pc), aux))) return rc;
            // The first chunk is swept in TWO parts only: everything but the last slice as soon as the last-but-one slice is prepared (beside the
            // last slice's copy), the last slice behind its own k_prep.  (Its exact sweep is a fixed ~0.5 ms of serial record loops per workgroup
            // whatever the number of pairs: one sweep per slice cost four times that on the main stream, 10.3 ms per step against 10.0.)
            const bool last = p0 + sl >= batch, last_but_one = !last && p0 + 2 * sl >= batch;
            if (last_but_one || last) HIPCHK(hipStreamWaitEvent(s, h->ev_prepped, 0)); // (the prep of this slice and, by stream order, of every slice before it)
            if (last_but_one) { swept0 = p0 + pc; if ((rc = first_chunk_of(0, swept0))) return rc; }
            if (last) { if ((rc = first_chunk_of(swept0, batch - swept0))) return rc; swept0 = batch; }
        }
        if (sliced) { HIPCHK(hipEventRecord(h->ev_solved[1], aux)); solved1 = true; }
        return MDRP_OK;
    }

    // Behind the super-chunk's last scan (chunk c): the LO of ALL its triggers, one persistent launch on aux2 (round 5: two launches, each with
    // its own tail of long problems, cost 4.3 ms where one costs 2.7; LO problems are independent of each other, so results are bit-identical).
    int lo(int c) {
        int32_t *lo_plan = h->work_pair.as<int32_t>();
        hipLaunchKernelGGL(k_lo_plan, dim3(1), dim3(PLAN_THREADS), 0, s, batch, h->st.as<PairState>(), (const int32_t *)nullptr, lo_plan);
        if (fuse_tail && !(front_cleared && fuse_cleared && it0 == 0)) {
            HIPCHK(hipMemsetAsync(fz_ctl, 0, 64 + 2 * sizeof(int32_t) * (size_t)batch, s));
            HIPCHK(hipMemsetAsync(fz_ready, 0xFF, sizeof(int32_t) * (size_t)batch, s));
        }
        if (piped) { HIPCHK(hipEventRecord(h->ev_scanned[c], s)); HIPCHK(hipStreamWaitEvent(aux2, h->ev_scanned[c], 0)); }
        const FuseTail fz = fuse_tail ? FuseTail{fz_done, fz_ready, fz_ctl, h->st.as<PairState>()} : FuseTail{nullptr, nullptr, nullptr, nullptr};
        unsigned long long *lm_stats = h->lm_stats.as<unsigned long long>();
        int32_t *xheads = cnt->xcd_head; // one LO queue per XCD (lo_take)
        hipEvent_t l0, l1; // HIP events on the stream the LO runs on (mdrp_stats::lo_ms)
        if (int rc = get_events(h, &l0, &l1, 2)) return rc;
        HIPCHK(hipEventRecord(l0, aux2));
        if (classic)
            MDRP_CLASSIC_LM_DISPATCH(kc_lo, lo_threads, kind, dim3(lo_blocks), clm_list_bytes, aux2, rp, h->st.as<PairState>(), h->pts.as<double>(),
                                     h->models.as<Model>(), h->triggers.as<Trigger>(), trig_cap, lo_plan, cnt->lo_head, xheads,
                                     h->lo_mask.as<uint8_t>(), clm_list_stride, fz);
        else
            MDRP_LM_DISPATCH(k_lo, lo_threads, kind, est_shift, dim3(lo_blocks), lm_list_bytes(n_max), aux2, rp,
                             h->st.as<PairState>(), h->pts.as<double>(), h->dep.as<double>(), h->models.as<Model>(), h->triggers.as<Trigger>(),
                             trig_cap, lo_plan, cnt->lo_head, xheads, lm_list_stride(n_max), lm_stats, fz);
        HIPCHK(hipEventRecord(l1, aux2));
        return MDRP_OK;
    }

    // `problems` final refinements on the main stream over the states `st_f` (run parameters `rf`): the pass's pairs, or the checkpoint problems of
    // a budgets call; the fused tail's (ready list, done flags, wait ticks, time-out counter), or (null, pairs to skip or null, 0, null)
    void final_of(const RunParams &rf, int problems, PairState *st_f, uint8_t *mask_f, ResultDev *results_f, const int32_t *ready, int32_t *fin_done,
                  unsigned long long ticks, unsigned long long *timeouts) {
        if (classic)
            MDRP_CLASSIC_LM_DISPATCH(kc_final, final_threads, kind, dim3(problems), clm_list_bytes, s, rf, st_f, h->pts.as<double>(), mask_f, results_f,
                                     ready, fin_done, ticks, timeouts, clm_list_stride);
        else
            MDRP_FINAL_DISPATCH(final_threads, rf.final_loss, kind, est_shift, dim3(problems), (mask_index ? lm_final_list_bytes(n_max) : lm_list_bytes(n_max)), s, rf,
                                st_f, h->pts.as<double>(), h->dep.as<double>(), mask_f, results_f, lm_list_stride(n_max), mask_index,
                                h->lm_stats.as<unsigned long long>() + 2, ready, fin_done, ticks, timeouts);
    }
    void final_pairs(const int32_t *ready, int32_t *fin_done, unsigned long long ticks, unsigned long long *timeouts) {
        final_of(rp, batch, h->st.as<PairState>(), mask_dev, results_dev, ready, fin_done, ticks, timeouts);
    }

    // fused tail: the final refinements on the main stream, released by k_gate when the last LO launch's queue is empty (bounded waits: mdrp_schedule.h)
    int gate_and_final() {
        const int32_t *plan_l = h->work_pair.as<int32_t>();
        const unsigned long long gate_ticks = 100ull * (unsigned long long)env_int("MDRP_FUSE_GATE_US", sched::fuse_gate_us(batch, n_max));
        const unsigned long long wait_ticks = 100ull * (unsigned long long)env_int("MDRP_FUSE_WAIT_US", sched::fuse_wait_us(batch, n_max));
        hipLaunchKernelGGL(k_gate, dim3(1), dim3(1), 0, s, (const int32_t *)cnt->lo_head, plan_l + 3 * (size_t)batch + 1,
                           (const int32_t *)fz_ctl, lo_blocks, gate_ticks, h->lm_stats.as<unsigned long long>() + 4);
        hipEvent_t g0, g1;
        if (int rc = get_events(h, &g0, &g1, 3)) return rc;
        HIPCHK(hipEventRecord(g0, s));
        final_pairs(fz_ready, fz_fin, wait_ticks, h->lm_stats.as<unsigned long long>() + 5);
        HIPCHK(hipEventRecord(g1, s));
        final_done = true;
        return MDRP_OK;
    }

    // replay of score_models / ransac bookkeeping over the ordered triggers (the fused tail's LO launch has done it; a budgets call takes its checkpoints here)
    int walk() {
        if (bud || !fuse_tail)
            launch_walk(s, batch, rp, h->st.as<PairState>(), h->models.as<Model>(), h->triggers.as<Trigger>(), trig_cap, &cnt->progress,
                        bud ? reinterpret_cast<const uint64_t *>(pd + sz.off_bud) : nullptr, n_bud, h->ckpt.as<PairState>());
        HIPCHK(hipGetLastError());
        return MDRP_OK;
    }

    // progress record: pairs still iterating, iterations they still need, evaluations swept (sum over pairs of models * n); the one host wait of a super-chunk
    int read_progress() {
        const Progress *pr = h->progress_host;
        HIPCHK(hipMemcpyAsync(h->progress_host, &cnt->progress, sizeof(Progress), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        h->sweep_evals += (int64_t)pr->evals;
        h->mfma_evals += (int64_t)pr->evals_mfma;
        h->fp64_evals += (int64_t)pr->evals_sweep;
        h->bound_evals += (int64_t)pr->evals_bound;
        if (final_done && pr->wish_pairs > 0) // (fused tail: the final refinements are behind this read-back; otherwise they are still to come)
            h->seen_wish[kind] = (double)pr->wish_sum / (double)pr->wish_pairs;
        if (getenv("MDRP_DEBUG"))
            fprintf(stderr, "[mdrp] super-chunk start %llu len %llu (%d chunks): evals %llu (mfma %llu, fp32 bound %llu, fp64 sweep %llu = %.2f %%) active %d max_needed %llu\n",
                    (unsigned long long)it0, (unsigned long long)lay.super_len, lay.n_chunks, pr->evals, pr->evals_mfma, pr->evals_bound, pr->evals_sweep,
                    100.0 * (double)pr->evals_sweep / (double)std::max<unsigned long long>(1, pr->evals), pr->n_active, pr->max_needed);
        return MDRP_OK;
    }

    // unfused: the final refinements of the pass's pairs, or of a budgets call's checkpoints, behind the last super-chunk
    int final_refinements() {
        hipEvent_t f0, f1;
        if (int rc = get_events(h, &f0, &f1, 3)) return rc;
        HIPCHK(hipEventRecord(f0, s));
        if (bud) {
            // the distinct checkpoint states of every pair in ONE launch over the compact list (k_ckpt_plan); every other checkpoint is filled from its
            // representative.  A pair that stops early, or whose best model does not change between two budgets, is refined once for all of them.
            const int problems = n_bud * batch;
            int32_t *list = h->ck_list.as<int32_t>(), *rep = list + problems, *done = rep + problems;
            hipLaunchKernelGGL(k_ckpt_plan, dim3(1), dim3(PLAN_THREADS), 0, s, batch, n_bud, h->ckpt.as<PairState>(), list, rep);
            RunParams rf = rp;
            rf.ck_pairs = batch; rf.ck_plane = bud->plane;
            rf.inl_stat = nullptr; // (the last budget's results alone feed the next call's first chunk: k_ckpt_fill)
            final_of(rf, problems, h->ckpt.as<PairState>(), bud->mask, bud->results, list, done, 0, nullptr);
            rf.inl_stat = rp.inl_stat;
            hipLaunchKernelGGL(k_ckpt_fill, dim3(problems), dim3(CKPT_FILL_THREADS), 0, s, rf, n_bud, h->ckpt.as<PairState>(), rep, bud->results, bud->mask);
        } else
            final_pairs(nullptr, nullptr, 0, nullptr);
        HIPCHK(hipEventRecord(f1, s));
        if (rp.inl_stat && h->wish_kind < 0) { // (the fused tail's sums came with the progress record; these arrive when the stream gets here: the next call looks)
            HIPCHK(hipMemcpyAsync(h->wish_host, rp.inl_stat, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIPCHK(hipEventRecord(h->ev_wish, s));
            h->wish_kind = kind;
        }
        HIPCHK(hipGetLastError());
        return MDRP_OK;
    }
};

// The stream schedule of a pass.  A super-chunk of several chunks is pipelined over three streams (the benchmark shape: 256 | 9744
// iterations); chunk c + 1 is solved while chunk c is swept, and the super-chunk has ONE LO launch, behind its last scan:
//   main:  clear prep solve0 count0 sort0 score0 scan0 | (wait solve1) count1 bound1 sort1 score1 scan1 | gate, final refinements (fused tail) | walk
//   aux :       (after prep; sched::second_solver_after) solve1 ...
//   aux2:  samples0 samples1 (beside prep)                                                        | (after the last scan) LO: ALL triggers of the super-chunk
// Host buffers of 512 pairs or more arrive in slices on a fourth stream (Pass::host_front):
//   copy:  slice0 slice1 slice2 slice3
//   aux :         prep0 solve1[0]  prep1 solve1[1]  prep2 solve1[2]  prep3 solve1[3]
//   main:                                          solve0 + sweep of chunk 0 [slices 0-2]   | solve0 + sweep of chunk 0 [slice 3] | count1 ...
// Otherwise (one chunk, or MDRP_LO_OVERLAP=0) aux and aux2 are the main stream and everything runs in the order it is issued.
int run_pass(mdrp_handle *h, const PassIn &in) {
    Pass p(h, in);
    hipStream_t s = p.s;
    int rc;
    if ((rc = p.plan_and_allocate()) || (rc = p.clear_front()) || (rc = p.upload_params())) return rc;
    HIPCHK(hipEventRecord(h->ev_tables, s)); // sample tables can be drawn from here on
    if (!p.host) { // device-resident inputs: everything is there (host buffers: the copies and k_prep are issued slice by slice by host_front)
        p.prep(0, p.batch, s);
        if (p.priors) p.prior();
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev_prepped, s)); // the records and pair states every solver reads are there from here on
    }
    p.rp.inl_stat = p.classic ? nullptr : &p.cnt->progress.wish_sum;

    uint64_t max_needed = 0;
    while (true) {
        if ((rc = p.begin_super_chunk(max_needed))) return rc;
        const int n_chunks = p.lay.n_chunks;
        const bool piped = p.piped;
        if (piped && p.it0 == 0 && (rc = p.presample())) return rc;
        bool solved1 = false; // the second chunk's solver has been issued (slice by slice)
        int swept0 = 0;       // pairs whose first chunk the sliced front has swept already
        if (p.host && p.it0 == 0 && (rc = p.host_front(solved1, swept0))) return rc;
        if (swept0 < p.batch && (rc = p.solve(p.view(0, 0, p.batch), s))) return rc;
        if (piped) HIPCHK(hipEventRecord(h->ev_solved[0], s));
        for (int c = 0; c < n_chunks; ++c) {
            p.rp.chunk_len = (int)p.lay.lens[c]; p.rp.chunk_off = p.lay.offs[c];
            if (c == 0 && swept0 >= p.batch) { // (the sliced front has swept the first chunk already)
                if (piped) HIPCHK(hipEventRecord(h->ev_scanned[0], s));
                continue;
            }
            if (piped && c + 1 < n_chunks && !(c == 0 && solved1)) {
                // the sampler tables advance in chunk order; chunk c + 1 reuses the lists chunk c - 1 was swept from
                // (the second chunk's solver needs nothing of the first one's: behind k_prep where sched::second_solver_after says so)
                const bool behind_prep = c == 0 && p.it0 == 0 &&
                    sched::second_solver_after(p.kind, p.presampled[1], p.host != nullptr, n_chunks, p.solve_behind_prep) == sched::SolveAfter::prep;
                HIPCHK(hipStreamWaitEvent(p.aux, c > 0 ? h->ev_scanned[c - 1] : (behind_prep ? h->ev_prepped : h->ev_solved[0]), 0));
                if ((rc = p.solve(p.view(c + 1, 0, p.batch), p.aux))) return rc;
                HIPCHK(hipEventRecord(h->ev_solved[c + 1], p.aux));
            }
            if (piped && c > 0) HIPCHK(hipStreamWaitEvent(s, h->ev_solved[c], 0));
            if (!piped && c > 0 && (rc = p.solve(p.view(c, 0, p.batch), s))) return rc;
            if ((rc = p.sweep(p.view(c, 0, p.batch)))) return rc;
            if (c + 1 < n_chunks) { // (the solver of chunk c + 2 waits for this chunk's scan: it reuses this chunk's lists)
                if (piped) HIPCHK(hipEventRecord(h->ev_scanned[c], s));
                continue;
            }
            if ((rc = p.lo(c))) return rc; // (records ev_scanned[c]; aux2 waits for it)
        }
        if (p.fuse_tail && (rc = p.gate_and_final())) return rc;
        if (piped) { HIPCHK(hipEventRecord(h->ev_lo, p.aux2)); HIPCHK(hipStreamWaitEvent(s, h->ev_lo, 0)); }
        if (p.fuse_tail) // behind the LO launch: the pairs a bounded wait gave up on (none in a healthy run: 1024 workgroups that read a flag)
            p.final_pairs(nullptr, p.fz_fin, 0, nullptr);
        if ((rc = p.walk()) || (rc = p.read_progress())) return rc;
        p.it0 += p.lay.super_len;
        if (h->progress_host->n_active == 0 || p.it0 >= p.ro->max_iterations) break;
        max_needed = h->progress_host->max_needed;
    }
    return p.final_done ? MDRP_OK : p.final_refinements(); // (fused tail: the final refinements ran beside the last LO launch)
}

// what every estimator call refuses before any device work
// the cameras a kind cannot run without (MDRP_SHARED_6PT reads the principal point from cam1 only)
const char *missing_cameras(int kind, int batch, const mdrp_camera *cam1, const mdrp_camera *cam2) {
    if (kind == MDRP_SHARED_6PT && batch > 0 && !cam1) return "the 6-point estimator needs the principal point in cam1";
    if ((kind == MDRP_CALIB || kind == MDRP_RELPOSE_5PT) && batch > 0 && (!cam1 || !cam2)) return "calibrated estimator needs cameras";
    return nullptr;
}

int estimate_refusals(mdrp_handle *h, const EstimateCall &c) {
    const bool known_kind = c.kind >= 0 && c.kind <= 5;
    if (!h || c.batch < 0 || c.n_max < 0 || !known_kind || !c.ro || !c.bo) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (const char *why = missing_cameras(c.kind, c.batch, c.cam1, c.cam2)) { g_err = why; return MDRP_ERR_INVALID; }
    if (c.kind <= 2 && c.batch > 0 && c.n_max > 0 && (!c.d1 || !c.d2)) { g_err = "monodepth estimator needs depths"; return MDRP_ERR_INVALID; }
    // RansacOptions switches of the reference that are not built are refused, never ignored (the reference would return different results)
    if (c.ro->progressive_sampling) { g_err = "progressive_sampling (PROSAC, RandomSampler::initialize_prosac) is not built on this entry point: it needs the match scores, mdrp_estimate_batch_ranked (scores= in Python) takes them"; return MDRP_ERR_UNSUPPORTED; }
    if (c.ro->real_focal_check && (c.kind == MDRP_SHARED_6PT || c.kind == MDRP_FUNDAMENTAL_7PT)) { g_err = "real_focal_check is not built"; return MDRP_ERR_UNSUPPORTED; }
    return MDRP_OK;
}

// Runs a call on the handle's streams: refusals, the handle's per-call state, the passes.  Returns with the work queued (a pass synchronises once per super-chunk).
int estimate_device(mdrp_handle *h, const EstimateCall &c) {
    const int kind = c.kind, batch = c.batch, n_max = c.n_max, n_budgets = c.n_budgets;
    const int32_t *n_per_pair = c.n_per_pair;
    const mdrp_ransac_opt *ro = c.ro;
    const uint64_t *budgets = c.budgets;
    if (int rc = estimate_refusals(h, c)) return rc;
    if (c.priors && (c.host || budgets)) { g_err = "priors: device-resident calls without budgets only"; return MDRP_ERR_INVALID; }
    if (c.prosac && (c.host || budgets || c.priors)) { g_err = "ranked: device-resident calls without budgets or priors only"; return MDRP_ERR_INVALID; }
    h->begin_call(batch, n_budgets);
    if (h->fuse_disabled && --h->fuse_retry_in <= 0) h->fuse_disabled = false; // once per API call (not per pass): the handle tries the fused tail again
    int rc;
    if ((rc = h->results.ensure(sizeof(ResultDev) * std::max(batch, 1)))) return rc;
    if ((rc = h->lm_stats.ensure(LM_STATS_BYTES))) return rc;
    // (device-resident inputs: the first pass clears the statistics with the rest of its front, Pass::clear_front)
    const bool stats_in_pass = front_clear_on() && batch > 0 && !c.host && !n_per_pair_out_of_range(n_per_pair, batch, n_max);
    if (!stats_in_pass) HIPCHK(hipMemsetAsync(h->lm_stats.p, 0, LM_STATS_BYTES, h->stream));
    if (batch == 0) return MDRP_OK;
    if (const char *why = n_per_pair_out_of_range(n_per_pair, batch, n_max)) { g_err = why; return MDRP_ERR_INVALID; } // (the plain entry points have no check before this one)
    std::vector<int32_t> n_host(batch);
    for (int i = 0; i < batch; ++i) n_host[i] = n_per_pair ? n_per_pair[i] : n_max;
    uint8_t *mask = c.mask_dev;
    if (!mask) {
        if ((rc = (budgets ? h->bmask : h->mask).ensure((size_t)std::max(n_budgets, 1) * batch * std::max(n_max, 1)))) return rc;
        mask = (budgets ? h->bmask : h->mask).as<uint8_t>();
    }
    // a budgets call: `mask` is [n_budgets][batch][n_max], the records go to the planes of `bresults` (allocated before the pass budget is taken
    // from the free memory below); the last plane is copied to `results` behind the passes
    if (budgets && (rc = h->bresults.ensure(sizeof(ResultDev) * n_budgets * batch))) return rc;
    // chunk capacity and pairs per pass from the scratch budget
    const int chunk_cap = sched::chunk_capacity(ro->max_iterations, ro->min_iterations);
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    // What one more pair adds to a pass's scratch (every buffer of a pass grows linearly with its pairs and its sample tables), with one sample table
    // per pair (a ragged batch may have as many).  Of the leading chunks, only the 5-point solver's second Reduce5 region depends on them.
    sched::Lead lead;
    const uint64_t lead0 = sched::parse_chunks(getenv("MDRP_CHUNKS"), lead) ? lead.first() : sched::LEAD_BUDGET;
    const size_t per_pair = pass_scratch(h, kind, 2, n_max, 2, chunk_cap, lead0, n_budgets).total() - pass_scratch(h, kind, 1, n_max, 1, chunk_cap, lead0, n_budgets).total();
    int per_pass = sched::pairs_per_pass(free_b, per_pair, batch);
    per_pass = std::max(1, std::min(per_pass, env_int("MDRP_PAIRS_PER_PASS", per_pass))); // (tests: several passes on a small batch)
    for (int p0 = 0; p0 < batch; p0 += per_pass) {
        const int nb = std::min(per_pass, batch - p0);
        const size_t o1 = (size_t)p0 * n_max, o2 = 2 * o1;
        HostSrc hs{};
        if (c.host) hs = HostSrc{c.host->x1 + o2, c.host->x2 + o2, c.host->d1 ? c.host->d1 + o1 : nullptr, c.host->d2 ? c.host->d2 + o1 : nullptr};
        const BudgetOut bud{budgets, n_budgets, h->bresults.as<ResultDev>() + p0, mask + o1, batch};
        PassIn in = pass_in(h, c, p0, nb, n_host.data() + p0, chunk_cap, mask + o1, c.host ? &hs : nullptr, budgets ? &bud : nullptr);
        in.clear_lm_stats = stats_in_pass && p0 == 0;
        if ((rc = run_pass(h, in))) return rc;
    }
    if (budgets) {
        HIPCHK(hipMemcpyAsync(h->results.p, h->bresults.as<ResultDev>() + (size_t)(n_budgets - 1) * batch, sizeof(ResultDev) * batch, hipMemcpyDeviceToDevice, h->stream));
    }
    return MDRP_OK;
}

int finish_timing(mdrp_handle *h) {
    if (h->lm_stats.p) HIPCHK(hipMemcpyAsync(h->lm_stats_host, h->lm_stats.p, LM_STATS_BYTES, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->lm_cost_evals = (int64_t)h->lm_stats_host[0]; h->lm_accum_evals = (int64_t)h->lm_stats_host[1];
    h->fin_cost_evals = (int64_t)h->lm_stats_host[2]; h->fin_accum_evals = (int64_t)h->lm_stats_host[3];
    h->fuse_gate_timeouts = (int64_t)h->lm_stats_host[4]; h->fuse_wait_timeouts = (int64_t)h->lm_stats_host[5];
    if (!(h->fuse_gate_timeouts || h->fuse_wait_timeouts) && !h->fuse_disabled) h->fuse_backoff = 64; // a clean call (fused or not needed): the back-off starts over
    if ((h->fuse_gate_timeouts || h->fuse_wait_timeouts) && !h->fuse_disabled) {
        // results are unaffected (the pass behind the LO launch refined what the waits gave up on), the call was slower than unfused.
        // Exponential back-off: 64, 128, ... 16384 unfused API calls after consecutive expired waits (a busy moment on a shared GPU costs 64 calls,
        // a profiler that serialises every dispatch soon costs nothing)
        h->fuse_disabled = true;
        h->fuse_retry_in = h->fuse_backoff;
        h->fuse_backoff = std::min(h->fuse_backoff * 2, 16384);
        if (!getenv("MDRP_QUIET"))
            fprintf(stderr, "[mdrp] fused tail: %lld gate / %lld final-refinement waits timed out (kernels of two streams did not overlap: "
                            "profiler or serialised dispatch?); this handle runs unfused for its next %d calls\n",
                    (long long)h->fuse_gate_timeouts, (long long)h->fuse_wait_timeouts, h->fuse_retry_in);
    }
    for (int k = 0; k < 6; ++k) { h->kind_ms[k] = 0; h->kind_launches[k] = 0; }
    for (size_t i = 0; i < h->ev_used; ++i) {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, h->ev_pool[i].first, h->ev_pool[i].second));
        const int k = std::min(std::max(h->ev_what[i], 0), 5);
        h->kind_ms[k] += t; h->kind_launches[k]++;
    }
    h->sweep_ms = h->kind_ms[0]; h->count_ms = h->kind_ms[1];
    return MDRP_OK;
}

} // namespace

// The one failure path behind MDRP_ENTER: a call that fails - a buffer that cannot grow, a HIP error, a helper's refusal - leaves through here whichever
// `return` it takes, and nothing of it stays in flight on the caller's buffers or the handle's: every stream of the handle is drained before the error
// is returned.  (A failure is what assigns g_err; a call that succeeds pays nothing.)
struct DrainOnFailure {
    mdrp_handle *const h;
    explicit DrainOnFailure(mdrp_handle *h_) : h(h_) { g_err.raised = false; }
    ~DrainOnFailure() {
        if (!g_err.raised) return;
        for (hipStream_t st : {h->stream, (hipStream_t)h->aux_stream, (hipStream_t)h->aux_stream2, (hipStream_t)h->copy_stream}) (void)hipStreamSynchronize(st);
    }
};

// serialise calls on one handle and run them on the handle's device; the caller's current device is restored on return; a failing call drains the handle
#define MDRP_ENTER(h)                                                                      \
    std::lock_guard<std::mutex> lock_((h)->mu);                                            \
    DeviceGuard guard_((h)->device);                                                       \
    if (!guard_.ok) { g_err = "hipSetDevice failed"; return MDRP_ERR_HIP; }                \
    DrainOnFailure drain_(h);

#ifndef MDRP_SRC_HASH
#define MDRP_SRC_HASH "unknown"
#endif

static int create_handle(int device, hipStream_t stream, bool own_stream, mdrp_handle **out);

extern "C" {

const char *mdrp_last_error(void) { return g_err.c_str(); }
// the build embeds a hash of the source files (mdrp_amd/build.py) so that a stale prebuilt library can be told from the tree
int mdrp_abi_version(void) { return MDRP_ABI_VERSION; }
const char *mdrp_version(void) { return "mdrp-hip 0.6 (gfx950) MDRP_SRC_HASH=" MDRP_SRC_HASH; }

// HIP_VERSION of the toolchain this library was compiled with (the runtime is bound at load time: mdrp_amd/_capi.py compares the two)
int mdrp_hip_build_version(void) { return HIP_VERSION; }

// the header's mdrp_create / mdrp_create_on_stream macros hand over the ABI the HOST was compiled against: another version, or another size of
// mdrp_ransac_opt, is refused here — before any call could read option fields past the end of a smaller struct
static int check_host_abi(int abi_version, int ransac_opt_bytes) {
    if (abi_version == MDRP_ABI_VERSION && ransac_opt_bytes == (int)sizeof(mdrp_ransac_opt)) return MDRP_OK;
    char buf[256];
    snprintf(buf, sizeof buf, "host was compiled against ABI %#x (mdrp_ransac_opt %d bytes), this library speaks %#x (%d bytes): recompile the host against include/mdrp.h",
             abi_version, ransac_opt_bytes, MDRP_ABI_VERSION, (int)sizeof(mdrp_ransac_opt));
    g_err = buf;
    return MDRP_ERR_INVALID;
}
int mdrp_create_(int device, void *stream, mdrp_handle **out, int abi_version, int ransac_opt_bytes) {
    if (int rc = check_host_abi(abi_version, ransac_opt_bytes)) return rc;
    return create_handle(device, (hipStream_t)stream, stream == nullptr, out);
}
int mdrp_create_on_stream_(int device, void *stream, mdrp_handle **out, int abi_version, int ransac_opt_bytes) {
    if (int rc = check_host_abi(abi_version, ransac_opt_bytes)) return rc;
    return create_handle(device, (hipStream_t)stream, false, out);
}

} // extern "C"

static int create_handle(int device, hipStream_t stream, bool own_stream, mdrp_handle **out) {
    if (!out) return MDRP_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        g_err = "no usable HIP device";
        return MDRP_ERR_NO_DEVICE;
    }
    DeviceGuard guard_(device);
    if (!guard_.ok) { g_err = "hipSetDevice failed"; return MDRP_ERR_HIP; }
    std::unique_ptr<mdrp_handle> h(new mdrp_handle()); // (a failed step below releases what the steps before it made)
    h->device = device;
    if (own_stream) HIPCHK(hipStreamCreateWithFlags(&h->own_stream.v, hipStreamNonBlocking));
    h->stream = own_stream ? h->own_stream.v : stream; // NULL here = the device's legacy default stream
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (prop.maxSharedMemoryPerMultiProcessor > 0) h->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor;
    HIPCHK(hipHostMalloc((void **)&h->progress_host.v, sizeof(Progress), hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&h->lm_stats_host.v, LM_STATS_BYTES, hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&h->wish_host.v, 2 * sizeof(int32_t), hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&h->ev_wish.v, hipEventDisableTiming));
    std::memset(h->lm_stats_host, 0, LM_STATS_BYTES);
    {   // high priority: the few long LO wavefronts should be placed first, the sweeps fill the remaining slots
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        HIPCHK(hipStreamCreateWithPriority(&h->aux_stream.v, hipStreamNonBlocking, prio_hi));
        HIPCHK(hipStreamCreateWithPriority(&h->aux_stream2.v, hipStreamNonBlocking, prio_hi));
    }
    HIPCHK(hipStreamCreateWithFlags(&h->copy_stream.v, hipStreamNonBlocking));
    for (Event *e : {&h->ev_copied, &h->ev_prepped, &h->ev_solved6, &h->ev_lo, &h->ev_tables, &h->ev_sampled[0], &h->ev_sampled[1]})
        HIPCHK(hipEventCreateWithFlags(&e->v, hipEventDisableTiming));
    for (int i = 0; i < sched::NC_MAX; ++i) {
        HIPCHK(hipEventCreateWithFlags(&h->ev_solved[i].v, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->ev_scanned[i].v, hipEventDisableTiming));
    }
    const int tile_bytes = (int)SCORE_TILE_BYTES;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_score<true>), hipFuncAttributeMaxDynamicSharedMemorySize, tile_bytes));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_score<false>), hipFuncAttributeMaxDynamicSharedMemorySize, tile_bytes));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_score<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, tile_bytes));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kc_solve5_reduce), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SOLVE5_LDS_BYTES));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kc_solver_unit<CLASSIC_RELPOSE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SOLVE5_LDS_BYTES));
    *out = h.release();
    return MDRP_OK;
}

// A probe's whole batch (r.batch pairs) as chunk 0 of a run: the scheduler's buffers from their start, parity 0.  (first_of_run is an input of the
// scheduler's decisions: no launcher reads it.)
static ChunkView probe_view(mdrp_handle *h, const RunParams &r) {
    ChunkView v;
    std::memset(&v, 0, sizeof v);
    v.pc = r.batch; v.r = r;
    v.st = h->st.as<PairState>(); v.pts = h->pts.as<double>(); v.models = h->models.as<Model>();
    v.slot_score = h->slot_score.as<double>(); v.slot_inl = h->slot_inl.as<int32_t>();
    v.tags = h->tags[0].as<uint32_t>(); v.tags_v = h->tags_v.as<uint32_t>();
    v.tags_sorted = h->tags_sorted[0].as<uint32_t>(); v.tags_sorted_other = h->tags_sorted[1].as<uint32_t>();
    v.model_count = h->model_count[0].as<int32_t>(); v.und_count = h->und_count.as<int32_t>();
    v.surv1 = h->surv_count.as<int32_t>(); v.surv2 = h->surv2_count.as<int32_t>();
    v.cand_stat = h->cand_stat.as<unsigned long long>(); v.rfrag = h->rfrag.as<uint4>(); v.trig = h->triggers.as<Trigger>();
    return v;
}

// The single-pair probes (mdrp_score_models, mdrp_count_candidates, mdrp_bound_models, retire_train) stage their pair as a one-pair chunk of `slots`
// slots per pair (the run parameters' slot_stride; chunk_len = ceil(num_models / 4) sizes the launchers' grids) and get its view `v`:
//   * the correspondences (host or device memory) packed into h->pts with their box, and the models;
//   * the pair's state: no records (nothing is pruned or retired: every model sees every correspondence) unless rec_score < DBL_MAX (retire_train);
//   * `listed` tags (`list`, or null: 0 .. num_models - 1) as the chunk's solver-order list with its count in model_count, or, as_survivors, as
//     k_count's survivors (tags_v, surv1); the other list counters cleared;
//   * frag: the records' MFMA fragments for k_count.
static int stage_unit_chunk(mdrp_handle *h, int kind, int mem_space, const mdrp_model *models, int num_models, size_t slots, const double *x1,
                            const double *x2, int n, double sq_threshold, const uint32_t *list, int listed, bool as_survivors, bool frag, ChunkView &v,
                            uint64_t rec_cnt = 0, double rec_score = DBL_MAX) {
    hipStream_t s = h->stream;
    const int nn = std::max(n, 1);
    const size_t tag_bytes = sizeof(uint32_t) * slots;
    const bool host = mem_space == MDRP_MEM_HOST;
    int rc;
    if ((rc = h->pts.ensure(sizeof(double) * PT_STRIDE * nn)) || (rc = h->st.ensure(sizeof(PairState))) ||
        (rc = h->models.ensure(sizeof(Model) * slots)) || (rc = h->slot_score.ensure(sizeof(double) * slots)) ||
        (rc = h->slot_inl.ensure(sizeof(int32_t) * slots)) || (rc = h->tags[0].ensure(tag_bytes)) || (rc = h->tags_v.ensure(tag_bytes)) ||
        (rc = h->tags_sorted[0].ensure(tag_bytes)) || (rc = h->tags_sorted[1].ensure(tag_bytes)) ||
        (rc = h->model_count[0].ensure(2 * sizeof(int32_t))) || (rc = h->und_count.ensure(2 * sizeof(int32_t))) ||
        (rc = h->surv_count.ensure(sizeof(int32_t))) || (rc = h->surv2_count.ensure(sizeof(int32_t))) ||
        (rc = h->cand_stat.ensure(2 * sizeof(unsigned long long))) || (rc = h->cplan.ensure(2 * sizeof(int32_t))) ||
        (rc = h->plan.ensure(sizeof(int32_t) * (2 + 2 + 4 + 16))) || (rc = h->rfrag.ensure((size_t)((nn + 15) / 16) * 1024)) ||
        (host && ((rc = h->in_x1.ensure(sizeof(double) * 2 * nn)) || (rc = h->in_x2.ensure(sizeof(double) * 2 * nn)))))
        return rc;
    RunParams rp;
    std::memset(&rp, 0, sizeof rp);
    rp.kind = kind; rp.batch = 1; rp.n_max = nn; rp.chunk_len = (num_models + 3) / 4; rp.super_len = rp.chunk_len; rp.slot_stride = (int)slots;
    rp.mps = 4; rp.sample_sz = 3;
    v = probe_view(h, rp);
    if (host) {
        HIPCHK(hipMemcpyAsync(h->in_x1.p, x1, sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(h->in_x2.p, x2, sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
        x1 = h->in_x1.as<double>(); x2 = h->in_x2.as<double>();
    }
    HIPCHK(hipMemcpyAsync(v.models, models, sizeof(Model) * num_models, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    std::vector<uint32_t> iota;
    if (!list) {
        iota.resize(listed = num_models);
        for (int i = 0; i < num_models; ++i) iota[i] = (uint32_t)i;
        list = iota.data();
    }
    const int32_t counts2[2] = {listed, 0}, surv = as_survivors ? listed : 0;
    HIPCHK(hipMemcpyAsync(as_survivors ? v.tags_v : v.tags, list, sizeof(uint32_t) * listed, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(v.model_count, counts2, sizeof counts2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(v.surv1, &surv, sizeof surv, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(v.surv2, 0, sizeof(int32_t), s));
    HIPCHK(hipMemsetAsync(v.und_count, 0, 2 * sizeof(int32_t), s));
    PairState ps;
    std::memset(&ps, 0, sizeof ps);
    ps.n = n; ps.active = 1; ps.sq_thr = sq_threshold; ps.eps = std::sqrt(sq_threshold);
    ps.best_min_cnt = rec_cnt; ps.best_min_score = rec_score < DBL_MAX ? rec_score : DBL_MAX; // (a NaN score is no record either)
    HIPCHK(hipMemcpyAsync(v.st, &ps, sizeof ps, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_pack_unit, dim3((n + 255) / 256 + 1), dim3(256), 0, s, n, x1, x2, (const double *)nullptr,
                       (const double *)nullptr, v.pts, (double *)nullptr);
    hipLaunchKernelGGL(k_box_unit, dim3(1), dim3(256), 0, s, n, v.pts, v.st);
    if (frag) hipLaunchKernelGGL(k_frag_unit, dim3((n + 16 + 255) / 256), dim3(256), 0, s, n, v.pts, v.rfrag);
    HIPCHK(hipStreamSynchronize(s)); // (the staged host copies go out of scope)
    return MDRP_OK;
}


static LmOpt lm_opt(const mdrp_bundle_opt *opt) {
    LmOpt o;
    o.max_it = (int)std::min<uint64_t>(opt->max_iterations, 1u << 30); o.loss = opt->loss_type; o.loss_scale = opt->loss_scale;
    o.grad_tol = opt->gradient_tol; o.step_tol = opt->step_tol; o.lambda0 = opt->initial_lambda;
    o.lambda_min = opt->min_lambda; o.lambda_max = opt->max_lambda;
    return o;
}

extern "C" {

void mdrp_destroy(mdrp_handle *h) {
    if (!h) return;
    DeviceGuard guard_(h->device);
    // no kernel or copy of the handle may still run when its memory goes: every stream first, then the handle, whose members free themselves
    // (a caller's stream is not the handle's to destroy)
    for (hipStream_t st : {h->stream, (hipStream_t)h->aux_stream, (hipStream_t)h->aux_stream2, (hipStream_t)h->copy_stream}) (void)hipStreamSynchronize(st);
    delete h;
}

int mdrp_synchronize(mdrp_handle *h) {
    if (!h) return MDRP_ERR_INVALID;
    MDRP_ENTER(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    return MDRP_OK;
}

} // extern "C"

// The estimator, refine, gather and rank entry points.  Each one is: refuse | fill the call record by name | run (blocking: stage, run, finish); the pieces
// are mdrp_capi_entry.h's.  A failure behind MDRP_ENTER drains the handle (DrainOnFailure): no entry point does it by hand.
#include "mdrp_capi_entry.h"

extern "C" {

// ---- the estimators, plain and with iteration budgets
int mdrp_estimate_batch_async(mdrp_handle *h, int kind, const double *x1, const double *x2, const double *d1, const double *d2,
                              int batch, int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2,
                              const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, uint8_t *inlier_mask_dev) {
    if (!h) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    EstimateCall c = call_of(kind, x1, x2, d1, d2, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    c.mask_dev = inlier_mask_dev;
    MDRP_ENTER(h);
    return estimate_device(h, c);
}

int mdrp_estimate_batch_budgets_async(mdrp_handle *h, int kind, const double *x1, const double *x2, const double *d1, const double *d2,
                                      int batch, int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2,
                                      const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, const uint64_t *budgets, int n_budgets,
                                      uint8_t *inlier_mask_dev) {
    if (!h) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (int rc = check_budgets(ropt, budgets, n_budgets)) return rc;
    EstimateCall c = call_of(kind, x1, x2, d1, d2, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    c.mask_dev = inlier_mask_dev; c.budgets = budgets; c.n_budgets = n_budgets;
    MDRP_ENTER(h);
    return estimate_device(h, c);
}

int mdrp_estimate_batch(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, const double *d1,
                        const double *d2, int batch, int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1,
                        const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, mdrp_result *out,
                        uint8_t *inlier_mask) {
    if (!h || !out || batch < 0 || n_max < 0) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    EstimateCall c = call_of(kind, x1, x2, d1, d2, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    return estimate_batch_blocking(h, c, mem_space, out, inlier_mask);
}

int mdrp_estimate_batch_budgets(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, const double *d1,
                                const double *d2, int batch, int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1,
                                const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, const uint64_t *budgets,
                                int n_budgets, mdrp_result *out, uint8_t *inlier_mask) {
    if (!h || !out || batch < 0 || n_max < 0) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (int rc = check_budgets(ropt, budgets, n_budgets)) return rc;
    EstimateCall c = call_of(kind, x1, x2, d1, d2, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    c.budgets = budgets; c.n_budgets = n_budgets;
    return estimate_batch_blocking(h, c, mem_space, out, inlier_mask);
}

int mdrp_copy_results_device(mdrp_handle *h, void *dst_dev, int batch) {
    if (!h || !dst_dev || batch < 0 || batch > h->last_batch) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    HIPCHK(hipMemcpyAsync(dst_dev, h->results.p, sizeof(ResultDev) * batch, hipMemcpyDeviceToDevice, h->stream));
    return finish_timing(h); // waits for the handle's stream: the records may be consumed on any other stream afterwards
}

int mdrp_fetch_results(mdrp_handle *h, mdrp_result *out, int batch) {
    if (!h) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    return fetch_results_locked(h, out, batch);
}

int mdrp_fetch_budget_results(mdrp_handle *h, mdrp_result *out, int n_budgets, int batch) {
    if (!h) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    return budget_results_locked(h, out, n_budgets, batch, hipMemcpyDeviceToHost);
}

int mdrp_copy_budget_results_device(mdrp_handle *h, void *dst_dev, int n_budgets, int batch) {
    if (!h) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    return budget_results_locked(h, dst_dev, n_budgets, batch, hipMemcpyDeviceToDevice); // (waits for the handle's stream, as mdrp_copy_results_device)
}

// ---- estimate with a prior
int mdrp_estimate_batch_prior_async(mdrp_handle *h, int kind, const double *x1, const double *x2, const double *d1, const double *d2, int batch, int n_max,
                                    const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt,
                                    const mdrp_bundle_opt *bopt, const mdrp_model *prior_dev, uint8_t *inlier_mask_dev) {
    EstimateCall c = call_of(kind, x1, x2, d1, d2, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    c.priors = reinterpret_cast<const Model *>(prior_dev); c.mask_dev = inlier_mask_dev;
    if (int rc = refuse(REFUSE_PRIOR, h, c, resident_args(prior_dev))) return rc;
    MDRP_ENTER(h);
    return estimate_device(h, c);
}

int mdrp_estimate_batch_prior(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, const double *d1, const double *d2, int batch,
                              int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt,
                              const mdrp_bundle_opt *bopt, const mdrp_model *prior, mdrp_result *out, uint8_t *inlier_mask) {
    EstimateCall c = call_of(kind, x1, x2, d1, d2, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    c.priors = reinterpret_cast<const Model *>(prior);
    if (int rc = refuse(REFUSE_PRIOR, h, c, blocking_args(mem_space, out, prior))) return rc;
    return run_blocking(h, c, mem_space, &c.priors, nullptr, out, inlier_mask, nullptr, [&] { return estimate_device(h, c); });
}

// ---- refine and verify caller-supplied models
int mdrp_refine_batch_async(mdrp_handle *h, int kind, const double *x1, const double *x2, const double *d1, const double *d2, int batch, int n_max,
                            const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt,
                            const mdrp_bundle_opt *bopt, const mdrp_model *models_dev, int stages, uint8_t *inlier_mask_dev, double *initial_score_dev,
                            int32_t *initial_inliers_dev) {
    EstimateCall c = call_of(kind, x1, x2, d1, d2, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    c.mask_dev = inlier_mask_dev;
    if (int rc = refuse(REFUSE_REFINE, h, c, resident_args(models_dev, stages))) return rc;
    MDRP_ENTER(h);
    return refine_device(h, c, reinterpret_cast<const Model *>(models_dev), stages, initial_score_dev, initial_inliers_dev);
}

int mdrp_refine_batch(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, const double *d1, const double *d2, int batch, int n_max,
                      const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                      const mdrp_model *models, int stages, mdrp_result *out, uint8_t *inlier_mask, double *initial_score, int32_t *initial_inliers) {
    EstimateCall c = call_of(kind, x1, x2, d1, d2, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    if (int rc = refuse(REFUSE_REFINE, h, c, blocking_args(mem_space, out, models, stages))) return rc;
    const Model *models_dev = reinterpret_cast<const Model *>(models);
    StartOutputs start{initial_score, initial_inliers};
    return run_blocking(h, c, mem_space, &models_dev, nullptr, out, inlier_mask, &start,
                        [&] { return refine_device(h, c, models_dev, stages, start.score_dev, start.inl_dev); });
}

// ---- the baselines from a caller's model
int mdrp_refine_classic_async(mdrp_handle *h, int kind, const double *x1, const double *x2, int batch, int n_max, const int32_t *n_per_pair,
                              const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                              const mdrp_model *models_dev, int stages, uint8_t *inlier_mask_dev, double *initial_score_dev, int32_t *initial_inliers_dev) {
    EstimateCall c = call_of(kind, x1, x2, nullptr, nullptr, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    c.mask_dev = inlier_mask_dev;
    if (int rc = refuse(REFUSE_REFINE_CLASSIC, h, c, resident_args(models_dev, stages))) return rc;
    MDRP_ENTER(h);
    return refine_classic_device(h, c, reinterpret_cast<const Model *>(models_dev), stages, initial_score_dev, initial_inliers_dev);
}

int mdrp_refine_classic(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, int batch, int n_max, const int32_t *n_per_pair,
                        const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, const mdrp_model *models,
                        int stages, mdrp_result *out, uint8_t *inlier_mask, double *initial_score, int32_t *initial_inliers) {
    EstimateCall c = call_of(kind, x1, x2, nullptr, nullptr, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    if (int rc = refuse(REFUSE_REFINE_CLASSIC, h, c, blocking_args(mem_space, out, models, stages))) return rc;
    const Model *models_dev = reinterpret_cast<const Model *>(models);
    StartOutputs start{initial_score, initial_inliers};
    return run_blocking(h, c, mem_space, &models_dev, nullptr, out, inlier_mask, &start,
                        [&] { return refine_classic_device(h, c, models_dev, stages, start.score_dev, start.inl_dev); });
}

int mdrp_estimate_classic_prior_async(mdrp_handle *h, int kind, const double *x1, const double *x2, int batch, int n_max, const int32_t *n_per_pair,
                                      const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                                      const mdrp_model *prior_dev, int prior_space, uint8_t *inlier_mask_dev) {
    EstimateCall c = call_of(kind, x1, x2, nullptr, nullptr, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    c.priors = reinterpret_cast<const Model *>(prior_dev); c.prior_space = prior_space; c.mask_dev = inlier_mask_dev;
    if (int rc = refuse(REFUSE_CLASSIC_PRIOR, h, c, resident_args(prior_dev))) return rc;
    MDRP_ENTER(h);
    return estimate_device(h, c);
}

int mdrp_estimate_classic_prior(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, int batch, int n_max, const int32_t *n_per_pair,
                                const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                                const mdrp_model *prior, int prior_space, mdrp_result *out, uint8_t *inlier_mask) {
    EstimateCall c = call_of(kind, x1, x2, nullptr, nullptr, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    c.priors = reinterpret_cast<const Model *>(prior); c.prior_space = prior_space;
    if (int rc = refuse(REFUSE_CLASSIC_PRIOR, h, c, blocking_args(mem_space, out, prior))) return rc;
    return run_blocking(h, c, mem_space, &c.priors, nullptr, out, inlier_mask, nullptr, [&] { return estimate_device(h, c); });
}

// ---- estimate in match-score order: the monodepth estimators, then the 5- / 6- / 7-point baselines (no depths)
int mdrp_estimate_batch_ranked_async(mdrp_handle *h, int kind, const double *x1, const double *x2, const double *d1, const double *d2, const double *scores_dev,
                                     int batch, int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2,
                                     const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, uint8_t *inlier_mask_dev) {
    EstimateCall c = call_of(kind, x1, x2, d1, d2, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    c.mask_dev = inlier_mask_dev;
    if (int rc = refuse(REFUSE_RANKED, h, c, resident_args())) return rc;
    MDRP_ENTER(h);
    return ranked_device(h, c, scores_dev);
}

int mdrp_estimate_batch_ranked(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, const double *d1, const double *d2,
                               const double *scores, int batch, int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2,
                               const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, mdrp_result *out, uint8_t *inlier_mask) {
    EstimateCall c = call_of(kind, x1, x2, d1, d2, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    if (int rc = refuse(REFUSE_RANKED, h, c, blocking_args(mem_space, out))) return rc;
    return run_blocking(h, c, mem_space, nullptr, &scores, out, inlier_mask, nullptr, [&] { return ranked_device(h, c, scores); });
}

int mdrp_estimate_classic_ranked_async(mdrp_handle *h, int kind, const double *x1, const double *x2, const double *scores_dev, int batch, int n_max,
                                       const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt,
                                       const mdrp_bundle_opt *bopt, uint8_t *inlier_mask_dev) {
    EstimateCall c = call_of(kind, x1, x2, nullptr, nullptr, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    c.mask_dev = inlier_mask_dev;
    if (int rc = refuse(REFUSE_CLASSIC_RANKED, h, c, resident_args())) return rc;
    MDRP_ENTER(h);
    return ranked_device(h, c, scores_dev);
}

int mdrp_estimate_classic_ranked(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, const double *scores, int batch, int n_max,
                                 const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt,
                                 const mdrp_bundle_opt *bopt, mdrp_result *out, uint8_t *inlier_mask) {
    EstimateCall c = call_of(kind, x1, x2, nullptr, nullptr, batch, n_max, n_per_pair, cam1, cam2, ropt, bopt);
    if (int rc = refuse(REFUSE_CLASSIC_RANKED, h, c, blocking_args(mem_space, out))) return rc;
    return run_blocking(h, c, mem_space, nullptr, &scores, out, inlier_mask, nullptr, [&] { return ranked_device(h, c, scores); });
}

// k_rank alone: order [batch][n_max] int32 in mem_space (-1 at and past n).  Synchronous.  (Not an estimator call: no record, its own three refusals.)
int mdrp_rank_scores(mdrp_handle *h, int mem_space, const double *scores, int batch, int n_max, const int32_t *n_per_pair, int32_t *order) {
    const char *why = nullptr;
    if (!h || batch < 0 || n_max < 0 || (mem_space != MDRP_MEM_HOST && mem_space != MDRP_MEM_DEVICE)) why = "invalid argument";
    else if ((size_t)batch * n_max > 0 && (!scores || !order)) why = "rank_scores: scores or order is NULL";
    else why = n_per_pair_out_of_range(n_per_pair, batch, n_max);
    if (why) { g_err = why; return MDRP_ERR_INVALID; }
    const size_t np = (size_t)batch * n_max;
    if (np == 0) return MDRP_OK;
    MDRP_ENTER(h);
    hipStream_t s = h->stream;
    const bool use_host = mem_space == MDRP_MEM_HOST;
    int rc;
    int32_t *order_dev = order;
    if (use_host) {
        if ((rc = h->pr_scores.ensure(sizeof(double) * np)) || (rc = h->pr_order.ensure(sizeof(int32_t) * np))) return rc;
        HIPCHK(hipMemcpyAsync(h->pr_scores.p, scores, sizeof(double) * np, hipMemcpyHostToDevice, s));
        scores = h->pr_scores.as<double>(); order_dev = h->pr_order.as<int32_t>();
    }
    if ((rc = rank_device(h, scores, batch, n_max, n_per_pair, order_dev))) return rc;
    if (use_host) HIPCHK(hipMemcpyAsync(order, order_dev, sizeof(int32_t) * np, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MDRP_OK;
}

// ---- the device front ends: sixteen entry points over four descriptors, each {gather | estimate} x {plain | ranked}
int mdrp_gather_matches(mdrp_handle *h, const mdrp_matches *mm, int batch, double *x1, double *x2, double *d1, double *d2, int32_t *slot,
                        int32_t *n_host) {
    return gather_alone(h, FE_MATCHES, mm, nullptr, MDRP_F64, batch, x1, x2, d1, d2, slot, n_host, "mdrp_gather_matches");
}
int mdrp_gather_matches_ranked(mdrp_handle *h, const mdrp_matches *mm, const void *scores_dev, int score_type, int batch, double *x1, double *x2, double *d1,
                               double *d2, int32_t *slot, int32_t *n_host) {
    return gather_alone(h, FE_MATCHES, mm, scores_dev, score_type, batch, x1, x2, d1, d2, slot, n_host, "mdrp_gather_matches_ranked");
}
int mdrp_gather_image_pairs(mdrp_handle *h, const mdrp_image_pairs *ip, int batch, double *x1, double *x2, double *d1, double *d2, int32_t *slot,
                            int32_t *n_host) {
    return gather_alone(h, FE_IMAGE_PAIRS, ip, nullptr, MDRP_F64, batch, x1, x2, d1, d2, slot, n_host, "mdrp_gather_image_pairs");
}
int mdrp_gather_image_pairs_ranked(mdrp_handle *h, const mdrp_image_pairs *ip, const void *scores_dev, int score_type, int batch, double *x1, double *x2,
                                   double *d1, double *d2, int32_t *slot, int32_t *n_host) {
    return gather_alone(h, FE_IMAGE_PAIRS, ip, scores_dev, score_type, batch, x1, x2, d1, d2, slot, n_host, "mdrp_gather_image_pairs_ranked");
}
int mdrp_gather_point_matches(mdrp_handle *h, const mdrp_point_matches *pm, int batch, double *x1, double *x2, int32_t *slot, int32_t *n_host) {
    return gather_alone(h, FE_POINT_MATCHES, pm, nullptr, MDRP_F64, batch, x1, x2, nullptr, nullptr, slot, n_host, "mdrp_gather_point_matches");
}
int mdrp_gather_point_matches_ranked(mdrp_handle *h, const mdrp_point_matches *pm, const void *scores_dev, int score_type, int batch, double *x1, double *x2,
                                     int32_t *slot, int32_t *n_host) {
    return gather_alone(h, FE_POINT_MATCHES, pm, scores_dev, score_type, batch, x1, x2, nullptr, nullptr, slot, n_host, "mdrp_gather_point_matches_ranked");
}
int mdrp_gather_point_image_pairs(mdrp_handle *h, const mdrp_point_image_pairs *pp, int batch, double *x1, double *x2, int32_t *slot, int32_t *n_host) {
    return gather_alone(h, FE_POINT_IMAGE_PAIRS, pp, nullptr, MDRP_F64, batch, x1, x2, nullptr, nullptr, slot, n_host, "mdrp_gather_point_image_pairs");
}
int mdrp_gather_point_image_pairs_ranked(mdrp_handle *h, const mdrp_point_image_pairs *pp, const void *scores_dev, int score_type, int batch, double *x1,
                                         double *x2, int32_t *slot, int32_t *n_host) {
    return gather_alone(h, FE_POINT_IMAGE_PAIRS, pp, scores_dev, score_type, batch, x1, x2, nullptr, nullptr, slot, n_host, "mdrp_gather_point_image_pairs_ranked");
}

int mdrp_estimate_matches_async(mdrp_handle *h, int kind, const mdrp_matches *mm, int batch, const mdrp_camera *cam1, const mdrp_camera *cam2,
                                const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, uint8_t *match_mask_dev, int32_t *n_used_host) {
    return estimate_front(h, FE_MATCHES, kind, mm, nullptr, MDRP_F64, false, batch, cam1, cam2, ropt, bopt, match_mask_dev, n_used_host, "mdrp_estimate_matches_async");
}
int mdrp_estimate_matches_ranked_async(mdrp_handle *h, int kind, const mdrp_matches *mm, const void *scores_dev, int score_type, int batch,
                                       const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                                       uint8_t *match_mask_dev, int32_t *n_used_host) {
    return estimate_front(h, FE_MATCHES, kind, mm, scores_dev, score_type, true, batch, cam1, cam2, ropt, bopt, match_mask_dev, n_used_host,
                          "mdrp_estimate_matches_ranked_async");
}
int mdrp_estimate_image_pairs_async(mdrp_handle *h, int kind, const mdrp_image_pairs *ip, int batch, const mdrp_camera *cam1, const mdrp_camera *cam2,
                                    const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, uint8_t *match_mask_dev, int32_t *n_used_host) {
    return estimate_front(h, FE_IMAGE_PAIRS, kind, ip, nullptr, MDRP_F64, false, batch, cam1, cam2, ropt, bopt, match_mask_dev, n_used_host,
                          "mdrp_estimate_image_pairs_async");
}
int mdrp_estimate_image_pairs_ranked_async(mdrp_handle *h, int kind, const mdrp_image_pairs *ip, const void *scores_dev, int score_type, int batch,
                                           const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                                           uint8_t *match_mask_dev, int32_t *n_used_host) {
    return estimate_front(h, FE_IMAGE_PAIRS, kind, ip, scores_dev, score_type, true, batch, cam1, cam2, ropt, bopt, match_mask_dev, n_used_host,
                          "mdrp_estimate_image_pairs_ranked_async");
}
int mdrp_estimate_classic_matches_async(mdrp_handle *h, int kind, const mdrp_point_matches *pm, int batch, const mdrp_camera *cam1, const mdrp_camera *cam2,
                                        const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, uint8_t *match_mask_dev, int32_t *n_used_host) {
    return estimate_front(h, FE_POINT_MATCHES, kind, pm, nullptr, MDRP_F64, false, batch, cam1, cam2, ropt, bopt, match_mask_dev, n_used_host,
                          "mdrp_estimate_classic_matches_async");
}
int mdrp_estimate_classic_matches_ranked_async(mdrp_handle *h, int kind, const mdrp_point_matches *pm, const void *scores_dev, int score_type, int batch,
                                               const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                                               uint8_t *match_mask_dev, int32_t *n_used_host) {
    return estimate_front(h, FE_POINT_MATCHES, kind, pm, scores_dev, score_type, true, batch, cam1, cam2, ropt, bopt, match_mask_dev, n_used_host,
                          "mdrp_estimate_classic_matches_ranked_async");
}
int mdrp_estimate_classic_image_pairs_async(mdrp_handle *h, int kind, const mdrp_point_image_pairs *pp, int batch, const mdrp_camera *cam1,
                                            const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, uint8_t *match_mask_dev,
                                            int32_t *n_used_host) {
    return estimate_front(h, FE_POINT_IMAGE_PAIRS, kind, pp, nullptr, MDRP_F64, false, batch, cam1, cam2, ropt, bopt, match_mask_dev, n_used_host,
                          "mdrp_estimate_classic_image_pairs_async");
}
int mdrp_estimate_classic_image_pairs_ranked_async(mdrp_handle *h, int kind, const mdrp_point_image_pairs *pp, const void *scores_dev, int score_type,
                                                   int batch, const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt,
                                                   const mdrp_bundle_opt *bopt, uint8_t *match_mask_dev, int32_t *n_used_host) {
    return estimate_front(h, FE_POINT_IMAGE_PAIRS, kind, pp, scores_dev, score_type, true, batch, cam1, cam2, ropt, bopt, match_mask_dev, n_used_host,
                          "mdrp_estimate_classic_image_pairs_ranked_async");
}

// ---- statistics of the last call, and the unit entry points
int mdrp_last_sweep_stats(mdrp_handle *h, double *sweep_ms, int64_t *launches, int64_t *evaluations) {
    if (!h) return MDRP_ERR_INVALID;
    std::lock_guard<std::mutex> lock_(h->mu);
    if (sweep_ms) *sweep_ms = h->sweep_ms;
    if (launches) *launches = h->sweep_launches;
    if (evaluations) *evaluations = h->sweep_evals;
    return MDRP_OK;
}

int mdrp_last_stats_sized(mdrp_handle *h, mdrp_stats *out, size_t out_size) {
    if (!h || !out || out_size < sizeof(double)) return MDRP_ERR_INVALID;
    std::lock_guard<std::mutex> lock_(h->mu);
    mdrp_stats full, *caller = out;
    out = &full;
    out->count_ms = h->count_ms; out->count_launches = h->count_launches;
    out->sweep_ms = h->sweep_ms; out->sweep_launches = h->sweep_launches;
    out->evals_algorithmic = h->sweep_evals; out->evals_mfma = h->mfma_evals; out->evals_fp64 = h->fp64_evals; out->evals_bound = h->bound_evals;
    out->lo_ms = h->kind_ms[2]; out->lo_launches = h->kind_launches[2]; out->final_ms = h->kind_ms[3]; out->final_launches = h->kind_launches[3];
    out->bound_ms = h->kind_ms[4]; out->bound_launches = h->kind_launches[4]; out->solve_ms = h->kind_ms[5]; out->solve_launches = h->kind_launches[5];
    out->lm_cost_evals = h->lm_cost_evals; out->lm_accum_evals = h->lm_accum_evals;
    out->final_cost_evals = h->fin_cost_evals; out->final_accum_evals = h->fin_accum_evals;
    out->fuse_gate_timeouts = h->fuse_gate_timeouts; out->fuse_wait_timeouts = h->fuse_wait_timeouts;
    out->first_chunk = h->first_chunk;
    std::memcpy(caller, &full, std::min(out_size, sizeof full)); // a caller compiled against an older, shorter struct gets its prefix
    return MDRP_OK;
}

// the round-3 entry point writes the round-3 struct (everything before fuse_gate_timeouts) and never more
int mdrp_last_stats(mdrp_handle *h, mdrp_stats *out) { return mdrp_last_stats_sized(h, out, offsetof(mdrp_stats, fuse_gate_timeouts)); }

int mdrp_solver_batch(mdrp_handle *h, int solver, const double *x1h, const double *x2h, const double *d1, const double *d2,
                      int count, mdrp_model *out, int32_t *n_out) {
    if (!h || count < 0 || solver < 0 || solver > 3 || !out || !n_out) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (count == 0) return MDRP_OK;
    MDRP_ENTER(h);
    int rc;
    if ((rc = h->unit_a.ensure(sizeof(double) * 9 * count)) || (rc = h->unit_b.ensure(sizeof(double) * 9 * count)) ||
        (rc = h->unit_c.ensure(sizeof(double) * 3 * count)) || (rc = h->unit_d.ensure(sizeof(double) * 3 * count)) ||
        (rc = h->unit_e.ensure(sizeof(Model) * 4 * count)) || (rc = h->unit_f.ensure(sizeof(int32_t) * count)))
        return rc;
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(h->unit_a.p, x1h, sizeof(double) * 9 * count, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->unit_b.p, x2h, sizeof(double) * 9 * count, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->unit_c.p, d1, sizeof(double) * 3 * count, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->unit_d.p, d2, sizeof(double) * 3 * count, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(h->unit_e.p, 0, sizeof(Model) * 4 * count, s));
    hipLaunchKernelGGL(k_solver_unit, dim3((count + 63) / 64), dim3(64), 0, s, solver, count, h->unit_a.as<double>(),
                       h->unit_b.as<double>(), h->unit_c.as<double>(), h->unit_d.as<double>(), h->unit_e.as<Model>(), h->unit_f.as<int32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->unit_e.p, sizeof(Model) * 4 * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_out, h->unit_f.p, sizeof(int32_t) * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MDRP_OK;
}

int mdrp_solver_residency(int device, int solver, int resident_per_simd, uint64_t keep_free_bytes, uint64_t *lds_per_cu, uint64_t *reserve_bytes,
                          int *workgroups_per_cu) {
    if (!lds_per_cu || !reserve_bytes || !workgroups_per_cu || solver < SOLVER_P3P || solver > SOLVER_VARYING) { g_err = "mdrp_solver_residency: bad argument"; return MDRP_ERR_INVALID; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) { g_err = "no usable HIP device"; return MDRP_ERR_NO_DEVICE; }
    DeviceGuard guard_(device);
    if (!guard_.ok) { g_err = "hipSetDevice failed"; return MDRP_ERR_HIP; }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    *lds_per_cu = (uint64_t)prop.maxSharedMemoryPerMultiProcessor;
    *reserve_bytes = (uint64_t)sched::solver_reservation((size_t)*lds_per_cu, resident_per_simd, (size_t)keep_free_bytes);
    const void *fn = solver == SOLVER_P3P ? reinterpret_cast<const void *>(k_solve<SOLVER_P3P>) : solver == SOLVER_SHIFT ? reinterpret_cast<const void *>(k_solve<SOLVER_SHIFT>)
                   : solver == SOLVER_SHARED ? reinterpret_cast<const void *>(k_solve<SOLVER_SHARED>) : reinterpret_cast<const void *>(k_solve<SOLVER_VARYING>);
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(workgroups_per_cu, fn, 64, (size_t)*reserve_bytes));
    return MDRP_OK;
}

int mdrp_classic_solver_batch(mdrp_handle *h, int kind, const double *x1h, const double *x2h, int count, mdrp_model *out, int32_t *n_out) {
    if (!h || count < 0 || kind < MDRP_RELPOSE_5PT || kind > MDRP_FUNDAMENTAL_7PT || !out || !n_out) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (count == 0) return MDRP_OK;
    MDRP_ENTER(h);
    const int K = kind == MDRP_RELPOSE_5PT ? 5 : (kind == MDRP_SHARED_6PT ? 6 : 7), M = kind == MDRP_RELPOSE_5PT ? MAX_MODELS_5PT : (kind == MDRP_SHARED_6PT ? MAX_MODELS_6PT : 3);
    int rc;
    if ((rc = h->unit_a.ensure(sizeof(double) * 3 * K * count)) || (rc = h->unit_b.ensure(sizeof(double) * 3 * K * count)) ||
        (rc = h->unit_e.ensure(sizeof(Model) * M * count)) || (rc = h->unit_f.ensure(sizeof(int32_t) * count)))
        return rc;
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(h->unit_a.p, x1h, sizeof(double) * 3 * K * count, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->unit_b.p, x2h, sizeof(double) * 3 * K * count, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(h->unit_e.p, 0, sizeof(Model) * M * count, s));
    if (kind == MDRP_SHARED_6PT)
        hipLaunchKernelGGL(kc_solver_unit<CLASSIC_SHARED>, dim3((count + 63) / 64), dim3(64), 0, s, count, h->unit_a.as<double>(),
                           h->unit_b.as<double>(), h->unit_e.as<Model>(), h->unit_f.as<int32_t>());
    else if (kind == MDRP_RELPOSE_5PT)
        hipLaunchKernelGGL(kc_solver_unit<CLASSIC_RELPOSE>, dim3((count + 63) / 64), dim3(64), SOLVE5_LDS_BYTES, s, count, h->unit_a.as<double>(),
                           h->unit_b.as<double>(), h->unit_e.as<Model>(), h->unit_f.as<int32_t>());
    else
        hipLaunchKernelGGL(kc_solver_unit<CLASSIC_FUND>, dim3((count + 63) / 64), dim3(64), SOLVE7_LDS_BYTES, s, count, h->unit_a.as<double>(),
                           h->unit_b.as<double>(), h->unit_e.as<Model>(), h->unit_f.as<int32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->unit_e.p, sizeof(Model) * M * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_out, h->unit_f.p, sizeof(int32_t) * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MDRP_OK;
}

// Exact scores of a model list as it stands: the one probe with a sweep launch of its own (k_score over the UNSORTED list, every model in the
// sparse class, on a grid capped at four workgroups per CU, so that the item loop runs), in slots padded to whole iterations of four.
int mdrp_score_models(mdrp_handle *h, int kind, int mem_space, const mdrp_model *models, int num_models, const double *x1,
                      const double *x2, int n, double sq_threshold, double *scores, int32_t *counts) {
    if (!h || num_models < 0 || n < 0 || kind < 0 || kind > 5 || !scores || !counts) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (num_models == 0) return MDRP_OK;
    MDRP_ENTER(h);
    hipStream_t s = h->stream;
    ChunkView v;
    int rc;
    if ((rc = stage_unit_chunk(h, kind, mem_space, models, num_models, (size_t)4 * ((num_models + 3) / 4), x1, x2, n, sq_threshold, nullptr, 0, false, false, v)))
        return rc;
    int32_t *plan = h->plan.as<int32_t>(), *totals = plan_totals(plan, 1);
    hipLaunchKernelGGL(k_plan, dim3(1), dim3(PLAN_THREADS), 0, s, 1, v.model_count, plan, totals, SCORE_THREADS);
    const dim3 grid((unsigned)std::min(h->num_cu * 4, (num_models + SCORE_THREADS - 1) / SCORE_THREADS));
    h->ev_used = 0; h->sweep_launches = 1; h->sweep_evals = (int64_t)num_models * n;
    hipEvent_t e0, e1;
    if ((rc = get_events(h, &e0, &e1))) return rc;
    HIPCHK(hipEventRecord(e0, s));
    MDRP_SWEEP_DISPATCH(k_score, kind, grid, dim3(SCORE_THREADS), SCORE_TILE_BYTES, s, v.r, v.st, v.pts, v.models, v.tags, v.model_count, v.slot_score,
                        v.slot_inl, plan, totals);
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipGetLastError());
    const hipMemcpyKind back = mem_space == MDRP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIPCHK(hipMemcpyAsync(scores, v.slot_score, sizeof(double) * num_models, back, s));
    HIPCHK(hipMemcpyAsync(counts, v.slot_inl, sizeof(int32_t) * num_models, back, s));
    return finish_timing(h);
}

// k_count's candidate counts of every model: the kernel's phase 0, the whole count in one launch with cand_out and no undecided lists, which
// no chunk of the scheduler runs: a launch of its own.
int mdrp_count_candidates(mdrp_handle *h, int kind, const mdrp_model *models, int num_models, const double *x1, const double *x2,
                          int n, double sq_threshold, int32_t *candidates) {
    if (!h || num_models < 0 || n < 0 || kind < 0 || kind > 5 || !candidates || !models) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (num_models == 0) return MDRP_OK;
    MDRP_ENTER(h);
    hipStream_t s = h->stream;
    ChunkView v;
    int rc;
    if ((rc = stage_unit_chunk(h, kind, MDRP_MEM_HOST, models, num_models, num_models, x1, x2, n, sq_threshold, nullptr, 0, false, true, v)) ||
        (rc = h->unit_f.ensure(sizeof(int32_t) * num_models)))
        return rc;
    int32_t *cplan = h->cplan.as<int32_t>();
    hipLaunchKernelGGL(k_count_plan, dim3(1), dim3(PLAN_THREADS), 0, s, 1, v.st, v.model_count, 2, CNT_WG_MODELS, cplan, (int32_t *)nullptr);
    const dim3 grid((unsigned)((num_models + CNT_WG_MODELS - 1) / CNT_WG_MODELS));
    MDRP_SWEEP_DISPATCH(k_count, kind, grid, dim3(CNT_THREADS), 0, s, v.r, v.st, v.rfrag, v.models, v.tags, v.model_count, cplan, v.tags_v, v.surv1,
                        (unsigned long long *)nullptr, h->unit_f.as<int32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(candidates, h->unit_f.p, sizeof(int32_t) * num_models, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MDRP_OK;
}

// k_bound's two bounds of every model, the models as k_count's survivors, through the scheduler's launcher.
int mdrp_bound_models(mdrp_handle *h, int kind, const mdrp_model *models, int num_models, const double *x1, const double *x2,
                      int n, double sq_threshold, double *score_lb, int32_t *count_ub) {
    if (!h || num_models < 0 || n < 0 || kind < 0 || kind > 5 || !score_lb || !count_ub || !models) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (num_models == 0) return MDRP_OK;
    MDRP_ENTER(h);
    hipStream_t s = h->stream;
    ChunkView v;
    Survivors sv;
    hipEvent_t b0, b1;
    int rc;
    if ((rc = stage_unit_chunk(h, kind, MDRP_MEM_HOST, models, num_models, num_models, x1, x2, n, sq_threshold, nullptr, 0, true, false, v)) ||
        (rc = h->unit_a.ensure(sizeof(double) * num_models)) || (rc = h->unit_f.ensure(sizeof(int32_t) * num_models)))
        return rc;
    HIPCHK(hipMemsetAsync(h->unit_a.p, 0, sizeof(double) * num_models, s));
    HIPCHK(hipMemsetAsync(h->unit_f.p, 0, sizeof(int32_t) * num_models, s));
    h->ev_used = 0;
    if ((rc = get_events(h, &b0, &b1, 4)) ||
        (rc = launch_bound(h, s, kind, v, nullptr, h->unit_a.as<double>(), h->unit_f.as<int32_t>(), b0, b1, sv)))
        return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(score_lb, h->unit_a.p, sizeof(double) * num_models, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(count_ub, h->unit_f.p, sizeof(int32_t) * num_models, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MDRP_OK;
}

// The armed stage train of one chunk on one pair, through the scheduler's own stage launchers (launch_count, launch_bound, launch_score) on the
// one-pair view of the handle's buffers: what the flags choose is what Pass::count, Pass::bound and Pass::score decide in a run.
// front_pick > 0 (mdrp_front_models): the train of a run's FIRST chunk instead — one count launch, no bound, the prefix retirement between the
// count and the sweep (launch_front), k_score.  Models with a NaN in their pose are then what k_solve's NaN model is: slot state -3, on no list.
static int retire_train(mdrp_handle *h, int kind, const mdrp_model *models, int num_models, const double *x1, const double *x2,
                        int n, double sq_threshold, uint64_t rec_cnt, double rec_score, const uint64_t *cand_stat_in, int flags, int front_pick,
                        double *scores, int32_t *counts, int32_t *left_at, int32_t *info, uint64_t *cand_stat_out) {
    const Sweep sweep = (flags & MDRP_RETIRE_SWEEP_WAVE) ? Sweep::wave : ((flags & MDRP_RETIRE_SWEEP_SPLIT) ? Sweep::split : Sweep::tile);
    const auto nan_pose = [](const mdrp_model &m) {
        return m.q[0] != m.q[0] || m.q[1] != m.q[1] || m.q[2] != m.q[2] || m.q[3] != m.q[3] || m.t[0] != m.t[0] || m.t[1] != m.t[1] || m.t[2] != m.t[2];
    };
    MDRP_ENTER(h);
    hipStream_t s = h->stream;
    const size_t slots = (size_t)num_models, tag_bytes = sizeof(uint32_t) * slots; // slot_stride = num_models: k_sort_tags writes the dense class from the back
    const bool armed = rec_score < DBL_MAX, two_phase = (flags & MDRP_RETIRE_TWO_PHASE) && armed; // (a run's first chunk has no record: no phase B)
    // every slot as k_solve leaves a live one: "no record" until an exact sweep writes it
    const std::vector<double> sc0(slots, DBL_MAX);
    std::vector<int32_t> in0(slots, -2);
    std::vector<uint32_t> list(slots);
    int listed = 0;
    for (int k = 0; k < num_models; ++k) {
        if (front_pick > 0 && nan_pose(models[k])) in0[k] = -3;
        else list[listed++] = (uint32_t)k;
    }
    ChunkView v;
    int rc;
    if ((rc = stage_unit_chunk(h, kind, MDRP_MEM_HOST, models, num_models, slots, x1, x2, n, sq_threshold, list.data(), listed, false, true, v, rec_cnt,
                               rec_score)) ||
        (rc = h->counters.ensure(sizeof(Counters))))
        return rc;
    const unsigned long long cs_in[2] = {cand_stat_in[0], cand_stat_in[1]};
    unsigned long long *front_evals = &h->counters.as<Counters>()->progress.evals_sweep;
    HIPCHK(hipMemcpyAsync(v.slot_score, sc0.data(), sizeof(double) * slots, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(v.slot_inl, in0.data(), sizeof(int32_t) * slots, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(v.cand_stat, cs_in, sizeof cs_in, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(h->counters.p, 0, sizeof(Counters), s));
    int32_t *plan = h->plan.as<int32_t>(), *totals = plan_totals(plan, 1);
    Survivors sv{v.tags_v, v.surv1};
    hipEvent_t c0, c1, b0, b1, f0, f1, e0, e1;
    h->ev_used = 0;
    // (a null cand_stat: the pair is never split)
    if ((rc = get_events(h, &c0, &c1, 1)) ||
        (rc = launch_count(h, s, kind, v, two_phase, nullptr, (flags & MDRP_RETIRE_TWO_PHASE) ? v.cand_stat : nullptr, c0, c1)))
        return rc;
    if ((flags & MDRP_RETIRE_BOUND) && ((rc = get_events(h, &b0, &b1, 4)) || (rc = launch_bound(h, s, kind, v, nullptr, nullptr, nullptr, b0, b1, sv))))
        return rc;
    if (front_pick > 0) {
        h->sweep_launches = 1; // (mdrp_front_models reports the front's sweep)
        if ((rc = get_events(h, &f0, &f1, 0)) || (rc = launch_front(h, s, kind, v, front_pick, plan, totals, front_evals, f0, f1, sv))) return rc;
    }
    if ((rc = get_events(h, &e0, &e1, 0)) || (rc = launch_score(h, s, kind, v, sv, sweep, plan, totals, e0, e1))) return rc;
    HIPCHK(hipGetLastError());
    // ---- the slots, and who left where: from the survivor lists of the two stages (tags_v and tags are not written behind the bound)
    const FrontLists f = front_lists(v);
    std::vector<uint32_t> list1(slots), list2(slots);
    int32_t n_und[2] = {0, 0}, n1 = 0, n2 = 0;
    unsigned long long cs_out[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(scores, v.slot_score, sizeof(double) * slots, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(counts, v.slot_inl, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(list1.data(), v.tags_v, tag_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(list2.data(), v.tags, tag_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_und, v.und_count, sizeof n_und, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&n1, v.surv1, sizeof n1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&n2, v.surv2, sizeof n2, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cs_out, v.cand_stat, sizeof cs_out, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const bool bound = (flags & MDRP_RETIRE_BOUND) != 0;
    if (front_pick > 0) {
        // the front's lists are where it left them (front_lists): the picked list is list2, the kept list list1; their counters n2, n_und[0] and n1
        std::vector<uint32_t> rest(slots);
        unsigned long long evals = 0;
        HIPCHK(hipMemcpyAsync(rest.data(), f.rest, tag_bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&evals, front_evals, sizeof evals, hipMemcpyDeviceToHost, s));
        if ((rc = finish_timing(h))) return rc;
        const int np = n2, nr = n_und[0];
        if (np < 0 || np > FIRST_PICK_MAX + 1 || nr < 0 || np + nr > listed || n1 < 0 || n1 > nr) { g_err = "front_models: list counts out of range"; return MDRP_ERR_INVALID; }
        for (int k = 0; k < num_models; ++k) left_at[k] = nan_pose(models[k]) ? 0 : 1; // (NaN models were on no list)
        for (int i = 0; i < nr; ++i) left_at[rest[i] & 0xFFFFFFu] = 5;
        for (int i = 0; i < n1; ++i) left_at[list1[i] & 0xFFFFFFu] = 3;
        for (int i = 0; i < np; ++i) left_at[list2[i] & 0xFFFFFFu] = 4;
        info[0] = np + nr; info[1] = np; info[2] = nr; info[3] = n1; info[4] = (int32_t)(evals / (unsigned long long)std::max(n, 1));
        return MDRP_OK;
    }
    if (n1 < 0 || n1 > num_models || n2 < 0 || n2 > n1) { g_err = "retire_models: survivor counts out of range"; return MDRP_ERR_INVALID; }
    for (int k = 0; k < num_models; ++k) left_at[k] = 1;
    for (int i = 0; i < n1; ++i) left_at[list1[i] & 0xFFFFFFu] = bound ? 2 : 3;
    if (bound) for (int i = 0; i < n2; ++i) left_at[list2[i] & 0xFFFFFFu] = 3;
    info[0] = n_und[0]; info[1] = n1; info[2] = bound ? n2 : n1;
    cand_stat_out[0] = cs_out[0]; cand_stat_out[1] = cs_out[1];
    return MDRP_OK;
}

int mdrp_retire_models(mdrp_handle *h, int kind, const mdrp_model *models, int num_models, const double *x1, const double *x2,
                       int n, double sq_threshold, uint64_t rec_cnt, double rec_score, const uint64_t *cand_stat_in, int flags,
                       double *scores, int32_t *counts, int32_t *left_at, int32_t *info, uint64_t *cand_stat_out) {
    const int sweep = flags & (MDRP_RETIRE_SWEEP_SPLIT | MDRP_RETIRE_SWEEP_WAVE);
    if (!h || num_models < 0 || num_models > 0xFFFFFF || n < 0 || kind < 0 || kind > 5 || !models || !cand_stat_in || !scores || !counts || !left_at ||
        !info || !cand_stat_out || (flags & ~15) || sweep == (MDRP_RETIRE_SWEEP_SPLIT | MDRP_RETIRE_SWEEP_WAVE)) {
        g_err = "invalid argument"; return MDRP_ERR_INVALID;
    }
    if (num_models == 0) return MDRP_OK;
    return retire_train(h, kind, models, num_models, x1, x2, n, sq_threshold, rec_cnt, rec_score, cand_stat_in, flags, 0, scores, counts, left_at, info,
                        cand_stat_out);
}

// The first chunk's train on one pair (include/mdrp.h): retire_train with the front between the count and k_score.
int mdrp_front_models(mdrp_handle *h, int kind, const mdrp_model *models, int num_models, const double *x1, const double *x2, int n,
                      double sq_threshold, uint64_t rec_cnt, double rec_score, int pick, double *scores, int32_t *counts, int32_t *left_at,
                      int32_t *info) {
    if (!h || num_models < 0 || num_models > 0xFFFFFF || n < 0 || kind < MDRP_CALIB || kind > MDRP_VARYING_FOCAL || !models || !x1 || !x2 || !scores ||
        !counts || !left_at || !info || pick < 1 || pick > sched::FIRST_PICK_LIMIT) {
        g_err = "front_models: a 3-point estimator, pick in 1..64 and no NULL buffer"; return MDRP_ERR_INVALID;
    }
    if (num_models == 0) return MDRP_OK;
    const uint64_t no_stat[2] = {0, 0};
    uint64_t stat_out[2];
    return retire_train(h, kind, models, num_models, x1, x2, n, sq_threshold, rec_cnt, rec_score, no_stat, MDRP_RETIRE_SWEEP_SCORE, pick, scores, counts,
                        left_at, info, stat_out);
}

// The bookkeeping train of one super-chunk on caller-given slot tables: the scan per chunk and the walk through the scheduler's own launchers
// (launch_scan, launch_walk), Pass::lo's plan kernel between them, with the scheduler's buffer roles (slots of chunk c at chunk_off * mps in the
// pair's slot row, triggers appended to the pair's list, the LO plan in work_pair, the progress record in the counter block, budgets in the params
// block, checkpoints in ckpt).  k_lo's part is played by the host.
int mdrp_replay_slots(mdrp_handle *h, const mdrp_ransac_opt *ro, mdrp_replay *io) {
    if (!h || !ro || !io) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    const int mps = io->mps, batch = io->batch, n_chunks = io->n_chunks, n_bud = io->budgets ? io->n_budgets : 0;
    const char *why = nullptr;
    long long super_ll = 0;
    if (mps != 4 && mps != 12 && mps != 16) why = "replay_slots: mps must be 4, 12 or 16";
    else if (io->sample_sz != 3 && io->sample_sz != 5 && io->sample_sz != 7) why = "replay_slots: sample_sz must be 3, 5 or 7";
    else if (batch < 1 || n_chunks < 1 || n_chunks > sched::NC_MAX || !io->chunk_lens) why = "replay_slots: batch >= 1 and 1 to 8 chunks";
    else {
        for (int c = 0; c < n_chunks; ++c) { if (io->chunk_lens[c] < 1) why = "replay_slots: a chunk length < 1"; super_ll += io->chunk_lens[c]; }
        if (!why && super_ll > (1 << 20)) why = "replay_slots: more than 2^20 iterations";
    }
    if (!why && (!io->slot_score || !io->slot_inl || !io->models || !io->lo_score || !io->lo_cnt || !io->lo_models || !io->states || !io->triggers ||
                 !io->n_triggers || !io->scan_cnt || !io->scan_score || !io->scan_inst || !io->lo_plan || !io->n_active || !io->max_needed ||
                 (n_bud && !io->checkpoints)))
        why = "replay_slots: a NULL buffer";
    if (!why && (io->n_budgets < 0 || n_bud > MAX_BUDGETS)) why = "replay_slots: more than MDRP_MAX_BUDGETS";
    for (int c = 0; c < n_bud && !why; ++c)
        if (io->budgets[c] < 1 || (c > 0 && io->budgets[c] <= io->budgets[c - 1]) || io->budgets[c] > ro->max_iterations)
            why = "replay_slots: budgets must be >= 1, strictly increasing and at most max_iterations";
    if (why) { g_err = why; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    hipStream_t s = h->stream;
    const int super_len = (int)super_ll, trig_cap = super_len;
    const size_t b = (size_t)batch, slots = b * super_len * mps, plan_ints = 3 * b + 2;
    int rc;
    if ((rc = h->st.ensure(sizeof(PairState) * b)) || (rc = h->models.ensure(sizeof(Model) * slots)) || (rc = h->slot_score.ensure(sizeof(double) * slots)) ||
        (rc = h->slot_inl.ensure(sizeof(int32_t) * slots)) || (rc = h->triggers.ensure(sizeof(Trigger) * b * trig_cap)) ||
        (rc = h->work_pair.ensure(sizeof(int32_t) * plan_ints)) || (rc = h->counters.ensure(sizeof(Counters))) ||
        (rc = h->model_count[0].ensure(sizeof(int32_t) * 2 * b)) || (rc = h->model_count[1].ensure(sizeof(int32_t) * 2 * b)) ||
        (rc = h->params.ensure(sizeof(uint64_t) * MAX_BUDGETS)) || (rc = h->ckpt.ensure(sizeof(PairState) * b * std::max(n_bud, 1))))
        return rc;
    std::vector<PairState> st_host(b), ck_host(b * n_bud);
    const auto stage = [](const mdrp_replay_state &z) {
        PairState ps;
        std::memset(&ps, 0, sizeof ps);
        ps.n = z.n; ps.active = z.active; ps.sq_thr = z.sq_thr; ps.eps = std::sqrt(z.sq_thr);
        ps.best_min_cnt = z.best_min_cnt; ps.best_min_score = z.best_min_score; ps.dyn_max_iter = z.dyn_max_iter; ps.iterations = z.iterations;
        ps.refinements = z.refinements; ps.num_inliers = z.num_inliers; ps.inlier_ratio = z.inlier_ratio; ps.model_score = z.model_score;
        std::memcpy(&ps.best, &z.best, sizeof(Model));
        return ps;
    };
    const auto unstage = [](const PairState &ps, mdrp_replay_state &z) {
        z.n = ps.n; z.active = ps.active; z.sq_thr = ps.sq_thr; z.best_min_cnt = ps.best_min_cnt; z.best_min_score = ps.best_min_score;
        z.dyn_max_iter = ps.dyn_max_iter; z.iterations = ps.iterations; z.refinements = ps.refinements; z.num_inliers = ps.num_inliers;
        z.inlier_ratio = ps.inlier_ratio; z.model_score = ps.model_score;
        std::memcpy(&z.best, &ps.best, sizeof(Model));
    };
    for (size_t p = 0; p < b; ++p) st_host[p] = stage(io->states[p]);
    for (size_t e = 0; e < ck_host.size(); ++e) ck_host[e] = stage(io->checkpoints[e]);
    PairState *st = h->st.as<PairState>();
    Trigger *trig = h->triggers.as<Trigger>();
    int32_t *lo_plan = h->work_pair.as<int32_t>();
    Counters *cnt = h->counters.as<Counters>();
    HIPCHK(hipMemcpyAsync(st, st_host.data(), sizeof(PairState) * b, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->models.p, io->models, sizeof(Model) * slots, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->slot_score.p, io->slot_score, sizeof(double) * slots, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->slot_inl.p, io->slot_inl, sizeof(int32_t) * slots, hipMemcpyHostToDevice, s));
    if (n_bud) {
        HIPCHK(hipMemcpyAsync(h->params.p, io->budgets, sizeof(uint64_t) * n_bud, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(h->ckpt.p, ck_host.data(), sizeof(PairState) * ck_host.size(), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemsetAsync(h->model_count[0].p, 0, sizeof(int32_t) * 2 * b, s));
    HIPCHK(hipMemsetAsync(h->model_count[1].p, 0, sizeof(int32_t) * 2 * b, s));
    HIPCHK(hipMemsetAsync(h->counters.p, 0, sizeof(Counters), s)); // (begin_super_chunk)
    RunParams rp;
    std::memset(&rp, 0, sizeof rp);
    rp.batch = batch; rp.n_max = 1; rp.mps = mps; rp.sample_sz = io->sample_sz; rp.slot_stride = super_len * mps; rp.super_len = super_len;
    rp.chunk_start = io->chunk_start; rp.max_iterations = ro->max_iterations; rp.min_iterations = ro->min_iterations;
    rp.dyn_mult = ro->dyn_num_trials_mult; rp.log_prob_missing = std::log(1.0 - ro->success_prob);
    // ---- Pass::scan, chunk by chunk; the pair states behind each scan travel back for the records and trigger counts
    std::vector<PairState> scanned(b * n_chunks);
    int off = 0;
    for (int c = 0; c < n_chunks; ++c) {
        RunParams r = rp;
        r.chunk_len = io->chunk_lens[c]; r.chunk_off = off;
        io->scan_inst[c] = launch_scan(s, mps, batch, r, st, h->slot_score.as<double>(), h->slot_inl.as<int32_t>(), trig, trig_cap,
                                       h->model_count[c & 1].as<int32_t>(), &cnt->progress.evals_sweep);
        HIPCHK(hipMemcpyAsync(scanned.data() + b * c, st, sizeof(PairState) * b, hipMemcpyDeviceToHost, s));
        off += io->chunk_lens[c];
    }
    rp.chunk_len = io->chunk_lens[n_chunks - 1]; rp.chunk_off = off - rp.chunk_len; // (as run_pass leaves them behind its chunk loop)
    // ---- Pass::lo: the plan; the LO itself is the caller's tables
    hipLaunchKernelGGL(k_lo_plan, dim3(1), dim3(PLAN_THREADS), 0, s, batch, st, (const int32_t *)nullptr, lo_plan);
    HIPCHK(hipGetLastError());
    std::vector<Trigger> trig_host(b * trig_cap);
    HIPCHK(hipMemcpyAsync(trig_host.data(), trig, sizeof(Trigger) * trig_host.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(io->lo_plan, lo_plan, sizeof(int32_t) * plan_ints, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int c = 0; c < n_chunks; ++c)
        for (size_t p = 0; p < b; ++p) {
            const PairState &ps = scanned[b * c + p];
            io->n_triggers[b * c + p] = ps.n_triggers; io->scan_cnt[b * c + p] = ps.best_min_cnt; io->scan_score[b * c + p] = ps.best_min_score;
        }
    for (size_t p = 0; p < b; ++p) {
        const int nt = scanned[b * (n_chunks - 1) + p].n_triggers;
        if (nt < 0 || nt > trig_cap) { g_err = "replay_slots: a trigger count outside the list"; return MDRP_ERR_INVALID; }
        for (int k = 0; k < nt; ++k) {
            Trigger &tr = trig_host[p * trig_cap + k];
            if (tr.iter >= (uint32_t)super_len || tr.k_ref < 0 || tr.k_ref >= mps || tr.k_min < -1 || tr.k_min >= mps) {
                g_err = "replay_slots: a trigger names a slot outside the tables"; return MDRP_ERR_INVALID;
            }
            const size_t slot = p * (size_t)rp.slot_stride + (size_t)tr.iter * mps + tr.k_ref;
            tr.ref_score = io->lo_score[slot]; tr.ref_cnt = io->lo_cnt[slot];
            std::memcpy(&tr.refined, &io->lo_models[slot], sizeof(Model));
            mdrp_replay_trigger &o = io->triggers[p * trig_cap + k];
            o.iter = tr.iter; o.k_ref = tr.k_ref; o.k_min = tr.k_min; o.cnt_min = tr.cnt_min; o.score_min = tr.score_min; o.cnt_ref = tr.cnt_ref; o.pad_ = 0;
        }
    }
    HIPCHK(hipMemcpyAsync(trig, trig_host.data(), sizeof(Trigger) * trig_host.size(), hipMemcpyHostToDevice, s));
    // ---- Pass::walk
    launch_walk(s, batch, rp, st, h->models.as<Model>(), trig, trig_cap, &cnt->progress, n_bud ? h->params.as<uint64_t>() : nullptr, n_bud,
                h->ckpt.as<PairState>());
    HIPCHK(hipGetLastError());
    // ---- Pass::read_progress, and the states
    Progress pr;
    HIPCHK(hipMemcpyAsync(&pr, &cnt->progress, sizeof pr, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(st_host.data(), st, sizeof(PairState) * b, hipMemcpyDeviceToHost, s));
    if (n_bud) HIPCHK(hipMemcpyAsync(ck_host.data(), h->ckpt.p, sizeof(PairState) * ck_host.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *io->n_active = pr.n_active; *io->max_needed = pr.max_needed;
    for (size_t p = 0; p < b; ++p) unstage(st_host[p], io->states[p]);
    for (size_t e = 0; e < ck_host.size(); ++e) unstage(ck_host[e], io->checkpoints[e]);
    return MDRP_OK;
}

// The front's pick and filter alone (launch_front_pick, launch_front_filter: the scheduler's own) on caller-given survivor lists and slot tables, in
// the front's lists (front_lists) of a view of the whole batch; the survivors arrive where the kept list will be (the filter overwrites what the
// pick has consumed).  k_first_score's part is played by the caller's tables.
static_assert(FIRST_PICK_MAX == sched::FIRST_PICK_LIMIT, "k_first_filter's LDS tables hold what the scheduler may pick");
int mdrp_front_lists(mdrp_handle *h, mdrp_front_tables *io) {
    if (!h || !io) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    const int batch = io->batch, slots = io->slots;
    const char *why = nullptr;
    if (batch < 1 || slots < 4 || slots % 4 || slots > (1 << 24)) why = "front_lists: batch >= 1 and 4 .. 2^24 slots per pair, a multiple of 4";
    else if (io->pick < 1 || io->pick > sched::FIRST_PICK_LIMIT) why = "front_lists: pick must be 1 .. 64";
    else if (!io->n || !io->active || !io->sq_thr || !io->count || !io->tags || !io->slot_score || !io->slot_inl || !io->tags_pick || !io->tags_rest ||
             !io->tags_out || !io->pick_count || !io->rest_count || !io->surv_count || !io->evals)
        why = "front_lists: a NULL buffer";
    for (int p = 0; p < batch && !why; ++p) {
        if (io->n[p] < 0 || io->count[p] < 0 || io->count[p] > slots) why = "front_lists: n or a list length out of range";
        for (int i = 0; !why && i < io->count[p]; ++i)
            if ((io->tags[(size_t)p * slots + i] & 0xFFFFFFu) >= (uint32_t)slots) why = "front_lists: a tag names a slot outside the table";
    }
    if (why) { g_err = why; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    hipStream_t s = h->stream;
    const size_t b = (size_t)batch, all = b * (size_t)slots, tag_bytes = sizeof(uint32_t) * all;
    int rc;
    if ((rc = h->st.ensure(sizeof(PairState) * b)) || (rc = h->slot_score.ensure(sizeof(double) * all)) || (rc = h->slot_inl.ensure(sizeof(int32_t) * all)) ||
        (rc = h->tags[0].ensure(tag_bytes)) || (rc = h->tags_v.ensure(tag_bytes)) || (rc = h->tags_sorted[1].ensure(tag_bytes)) ||
        (rc = h->surv_count.ensure(sizeof(int32_t) * b)) || (rc = h->surv2_count.ensure(sizeof(int32_t) * b)) ||
        (rc = h->und_count.ensure(sizeof(int32_t) * 2 * b)) || (rc = h->counters.ensure(sizeof(Counters))))
        return rc;
    std::vector<PairState> st_host(b);
    int n_max = 1;
    for (size_t p = 0; p < b; ++p) {
        PairState &ps = st_host[p];
        std::memset(&ps, 0, sizeof ps);
        ps.n = io->n[p]; ps.active = io->active[p]; ps.sq_thr = io->sq_thr[p]; ps.eps = std::sqrt(io->sq_thr[p]); ps.best_min_score = DBL_MAX;
        n_max = std::max(n_max, ps.n);
    }
    RunParams rp;
    std::memset(&rp, 0, sizeof rp);
    rp.batch = batch; rp.n_max = n_max; rp.chunk_len = slots / 4; rp.super_len = rp.chunk_len; rp.slot_stride = slots; rp.mps = 4; rp.sample_sz = 3;
    const ChunkView v = probe_view(h, rp);
    const FrontLists f = front_lists(v);
    unsigned long long *evals = &h->counters.as<Counters>()->progress.evals_sweep;
    HIPCHK(hipMemcpyAsync(v.st, st_host.data(), sizeof(PairState) * b, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(v.slot_score, io->slot_score, sizeof(double) * all, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(v.slot_inl, io->slot_inl, sizeof(int32_t) * all, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(f.kept, io->tags, tag_bytes, hipMemcpyHostToDevice, s)); // (k_count's survivors, where the kept list will be)
    HIPCHK(hipMemcpyAsync(f.n_kept, io->count, sizeof(int32_t) * b, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(f.pick, io->tags_pick, tag_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(f.rest, io->tags_rest, tag_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(f.n_pick, io->pick_count, sizeof(int32_t) * b, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(f.n_rest, io->rest_count, sizeof(int32_t) * 2 * b, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(h->counters.p, 0, sizeof(Counters), s));
    launch_front_pick(s, v, Survivors{f.kept, f.n_kept}, io->pick);
    // the pick has consumed the survivors: what the caller put into the kept list and its counter takes their place, so that an inactive pair's stay
    HIPCHK(hipMemcpyAsync(f.kept, io->tags_out, tag_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(f.n_kept, io->surv_count, sizeof(int32_t) * b, hipMemcpyHostToDevice, s));
    (void)launch_front_filter(s, v, evals);
    HIPCHK(hipGetLastError());
    unsigned long long ev = 0;
    HIPCHK(hipMemcpyAsync(io->tags_pick, f.pick, tag_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(io->tags_rest, f.rest, tag_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(io->tags_out, f.kept, tag_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(io->pick_count, f.n_pick, sizeof(int32_t) * b, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(io->rest_count, f.n_rest, sizeof(int32_t) * 2 * b, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(io->surv_count, f.n_kept, sizeof(int32_t) * b, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&ev, evals, sizeof ev, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *io->evals = ev;
    return MDRP_OK;
}

// The front of a pass up to and including each chunk's solver, stage for stage what run_pass issues for device-resident inputs: Pass::plan / allocate,
// upload_params, prep, begin_super_chunk on the caller's chunks, presample where the super-chunk is pipelined, then Pass::solve on view(c, 0, batch) chunk
// by chunk on the main stream.  Between the stages the handle's buffers are only filled with MDRP_FRONT_FILL and read back.
static_assert(sizeof(mdrp_front_state) == sizeof(PairState) && offsetof(mdrp_front_state, norm) == offsetof(PairState, norm) &&
                  offsetof(mdrp_front_state, cen) == offsetof(PairState, cen) && offsetof(mdrp_front_state, dyn_max_iter) == offsetof(PairState, dyn_max_iter) &&
                  offsetof(mdrp_front_state, best) == offsetof(PairState, best),
              "mdrp_front_state mirrors PairState");
int mdrp_front_stages(mdrp_handle *h, const mdrp_ransac_opt *ro, const mdrp_bundle_opt *bo, mdrp_front_run *io) {
    if (!h || !io) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    EstimateCall c = call_of(io->kind, io->x1, io->x2, io->d1, io->d2, io->batch, io->n_max, io->n_per_pair, io->cam1, io->cam2, ro, bo);
    if (int rc = estimate_refusals(h, c)) return rc;
    const int kind = io->kind, batch = io->batch, n_max = io->n_max, n_chunks = io->n_chunks;
    const bool mono = kind <= MDRP_VARYING_FOCAL;
    if (!mono) c.d1 = c.d2 = nullptr; // (a baseline takes no depths)
    const char *why = nullptr;
    long long super_ll = 0;
    if (batch < 1 || n_max < 1 || !io->x1 || !io->x2) why = "front_stages: batch >= 1, n_max >= 1 and the correspondences";
    else if (n_chunks < 1 || n_chunks > sched::NC_MAX || !io->chunk_lens) why = "front_stages: 1 to 8 chunks";
    else if (!io->pts || (mono && !io->dep) || !io->rfrag || !io->states || !io->table_of_pair || !io->table_n || !io->n_tables || !io->samples ||
             !io->slot_inl || !io->models || !io->tags || !io->model_count)
        why = "front_stages: a NULL output";
    else why = n_per_pair_out_of_range(io->n_per_pair, batch, n_max);
    for (int k = 0; !why && k < n_chunks; ++k) { if (io->chunk_lens[k] < 1) why = "front_stages: a chunk length < 1"; super_ll += io->chunk_lens[k]; }
    const int chunk_cap = why ? 0 : sched::chunk_capacity(ro->max_iterations, ro->min_iterations);
    if (!why && (super_ll > chunk_cap || io->slot_iters < super_ll || io->slot_iters > chunk_cap))
        why = "front_stages: the chunks and slot_iters must fit the pass's capacity (sched::chunk_capacity), slot_iters >= the sum of the chunks";
    if (why) { g_err = why; return MDRP_ERR_INVALID; }
    std::vector<int32_t> n_host(batch);
    for (int i = 0; i < batch; ++i) n_host[i] = io->n_per_pair ? io->n_per_pair[i] : n_max;
    sched::Layout lay;
    lay.n_chunks = n_chunks;
    for (int k = 0; k < n_chunks; ++k) { lay.lens[k] = (uint64_t)io->chunk_lens[k]; lay.super_len += lay.lens[k]; }
    for (int k = 1; k < n_chunks; ++k) lay.offs[k] = lay.offs[k - 1] + (int)lay.lens[k - 1];
    const int super_len = (int)super_ll;

    MDRP_ENTER(h);
    Pass p(h, pass_in(h, c, 0, batch, n_host.data(), chunk_cap, nullptr, nullptr, nullptr));
    p.plan();
    // what Pass::solve would refuse in the middle of the run
    if (kind == MDRP_RELPOSE_5PT && n_chunks > 1 && (lay.lens[0] + 63) / 64 > p.sz.red5_first_blocks) {
        g_err = "front_stages: 5-point first chunk longer than its Reduce5 region"; return MDRP_ERR_INVALID;
    }
    hipStream_t s = p.s;
    int rc;
    h->ev_used = 0;
    if ((rc = stage_host_call(h, c, nullptr, nullptr))) return rc;
    p.x1 = c.x1; p.x2 = c.x2; p.d1 = c.d1; p.d2 = c.d2;
    if ((rc = p.allocate()) || (rc = p.upload_params())) return rc;
    const size_t b = (size_t)batch, slots = b * p.rp.slot_stride, mps = (size_t)p.mps, ssz = (size_t)p.ssz;
    const size_t smp_words = ssz * p.n_tables * chunk_cap;
    const size_t np = b * n_max, frag_words = b * p.groups_max * 64 * 4;
    HIPCHK(hipMemsetAsync(h->pts.p, MDRP_FRONT_FILL, sizeof(double) * PT_STRIDE * np, s));
    if (mono) HIPCHK(hipMemsetAsync(h->dep.p, MDRP_FRONT_FILL, sizeof(double) * 2 * np, s));
    HIPCHK(hipMemsetAsync(h->rfrag.p, MDRP_FRONT_FILL, sizeof(uint32_t) * frag_words, s));
    HIPCHK(hipMemsetAsync(h->models.p, MDRP_FRONT_FILL, sizeof(Model) * slots, s));
    HIPCHK(hipMemsetAsync(h->slot_inl.p, MDRP_FRONT_FILL, sizeof(int32_t) * slots, s));
    for (int q = 0; q < 2; ++q) {
        HIPCHK(hipMemsetAsync(h->samples[q].p, MDRP_FRONT_FILL, sizeof(uint32_t) * smp_words, s));
        HIPCHK(hipMemsetAsync(h->tags[q].p, MDRP_FRONT_FILL, sizeof(uint32_t) * slots, s));
    }
    HIPCHK(hipEventRecord(h->ev_tables, s));
    p.prep(0, batch, s);
    HIPCHK(hipGetLastError());
    // ---- behind the prep
    std::vector<PairState> st_host(b);
    HIPCHK(hipMemcpyAsync(io->pts, h->pts.p, sizeof(double) * PT_STRIDE * np, hipMemcpyDeviceToHost, s));
    if (mono) HIPCHK(hipMemcpyAsync(io->dep, h->dep.p, sizeof(double) * 2 * np, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(io->rfrag, h->rfrag.p, sizeof(uint32_t) * frag_words, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(st_host.data(), h->st.p, sizeof(PairState) * b, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::memcpy(io->states, st_host.data(), sizeof(PairState) * b);
    std::memcpy(io->table_of_pair, p.table_of.data(), sizeof(int32_t) * b);
    std::memcpy(io->table_n, p.tab_n.data(), sizeof(int32_t) * p.n_tables);
    *io->n_tables = p.n_tables;
    // ---- the chunks
    if ((rc = p.begin_super_chunk(lay))) return rc;
    if (p.piped && (rc = p.presample())) return rc;
    const size_t out_slots = (size_t)io->slot_iters * mps;
    std::vector<uint32_t> smp_host(smp_words), tags_host(slots);
    std::vector<int32_t> inl_host(slots);
    for (int k = 0; k < n_chunks; ++k) {
        const ChunkView v = p.view(k, 0, batch);
        const size_t len = (size_t)lay.lens[k];
        if (!(k < 2 && p.presampled[k])) HIPCHK(hipMemsetAsync(v.samples, MDRP_FRONT_FILL, sizeof(uint32_t) * smp_words, s));
        if (k >= 2) HIPCHK(hipMemsetAsync(v.tags, MDRP_FRONT_FILL, sizeof(uint32_t) * slots, s));
        if ((rc = p.solve(v, s))) return rc;
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(smp_host.data(), v.samples, sizeof(uint32_t) * ssz * p.n_tables * len, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(tags_host.data(), v.tags, sizeof(uint32_t) * slots, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(inl_host.data(), v.slot_inl, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(io->model_count + 2 * b * k, v.model_count, sizeof(int32_t) * 2 * b, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int t = 0; t < p.n_tables; ++t)
            std::memcpy(io->samples + ((size_t)t * super_len + lay.offs[k]) * ssz, smp_host.data() + (size_t)t * len * ssz, sizeof(uint32_t) * len * ssz);
        for (size_t q = 0; q < b; ++q) {
            std::memcpy(io->tags + (b * k + q) * out_slots, tags_host.data() + q * p.rp.slot_stride, sizeof(uint32_t) * out_slots);
            std::memcpy(io->slot_inl + (b * k + q) * out_slots, inl_host.data() + q * p.rp.slot_stride, sizeof(int32_t) * out_slots);
        }
    }
    std::vector<Model> models_host(slots);
    HIPCHK(hipMemcpyAsync(models_host.data(), h->models.p, sizeof(Model) * slots, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (hipStream_t st : {(hipStream_t)h->aux_stream, (hipStream_t)h->aux_stream2}) HIPCHK(hipStreamSynchronize(st));
    for (size_t q = 0; q < b; ++q) std::memcpy(io->models + q * out_slots, models_host.data() + q * p.rp.slot_stride, sizeof(Model) * out_slots);
    return MDRP_OK;
}

int mdrp_refine_models(mdrp_handle *h, int kind, mdrp_model *models, int count, const double *x1, const double *x2,
                       const double *d1, const double *d2, int n, double scale_reproj, double weight_sampson,
                       const mdrp_bundle_opt *opt, int estimate_shift, double *final_cost) {
    if (!h || count < 0 || n < 0 || kind < 0 || kind > 5 || !opt || !models) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (count == 0) return MDRP_OK;
    MDRP_ENTER(h);
    hipStream_t s = h->stream;
    int rc;
    const int nn = std::max(n, 1);
    if (kind >= MDRP_RELPOSE_5PT) {
        if ((rc = h->pts.ensure(sizeof(double) * PT_STRIDE * nn)) || (rc = h->in_x1.ensure(sizeof(double) * 2 * nn)) ||
            (rc = h->in_x2.ensure(sizeof(double) * 2 * nn)) || (rc = h->unit_e.ensure(sizeof(Model) * count)) ||
            (rc = h->unit_a.ensure(sizeof(double) * count)))
            return rc;
        HIPCHK(hipMemcpyAsync(h->in_x1.p, x1, sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(h->in_x2.p, x2, sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(h->unit_e.p, models, sizeof(Model) * count, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_pack_unit, dim3((n + 255) / 256 + 1), dim3(256), 0, s, n, h->in_x1.as<double>(), h->in_x2.as<double>(),
                           (const double *)nullptr, (const double *)nullptr, h->pts.as<double>(), (double *)nullptr);
        MDRP_CLASSIC_LM_DISPATCH(kc_refine_unit, (count >= 2048 ? 64 : 256), kind, dim3(count), 0, s, count, h->unit_e.as<Model>(),
                                 h->pts.as<double>(), n, lm_opt(opt), h->unit_a.as<double>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(models, h->unit_e.p, sizeof(Model) * count, hipMemcpyDeviceToHost, s));
        if (final_cost) HIPCHK(hipMemcpyAsync(final_cost, h->unit_a.p, sizeof(double) * count, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return MDRP_OK;
    }
    if ((rc = h->pts.ensure(sizeof(double) * PT_STRIDE * nn)) || (rc = h->dep.ensure(sizeof(double) * 2 * nn)) ||
        (rc = h->in_x1.ensure(sizeof(double) * 2 * nn)) || (rc = h->in_x2.ensure(sizeof(double) * 2 * nn)) ||
        (rc = h->in_d1.ensure(sizeof(double) * nn)) || (rc = h->in_d2.ensure(sizeof(double) * nn)) ||
        (rc = h->unit_e.ensure(sizeof(Model) * count)) || (rc = h->unit_a.ensure(sizeof(double) * count)))
        return rc;
    HIPCHK(hipMemcpyAsync(h->in_x1.p, x1, sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->in_x2.p, x2, sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->in_d1.p, d1, sizeof(double) * n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->in_d2.p, d2, sizeof(double) * n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->unit_e.p, models, sizeof(Model) * count, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_pack_unit, dim3((n + 255) / 256 + 1), dim3(256), 0, s, n, h->in_x1.as<double>(), h->in_x2.as<double>(),
                       h->in_d1.as<double>(), h->in_d2.as<double>(), h->pts.as<double>(), h->dep.as<double>());
    MDRP_LM_DISPATCH(k_refine_unit, (count >= 2048 ? 64 : 256), kind, (kind == MDRP_CALIB && estimate_shift), dim3(count), lm_list_bytes(n), s,
                     count, h->unit_e.as<Model>(), h->pts.as<double>(), h->dep.as<double>(), n, scale_reproj, weight_sampson, lm_opt(opt),
                     h->unit_a.as<double>(), lm_list_stride(n));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(models, h->unit_e.p, sizeof(Model) * count, hipMemcpyDeviceToHost, s));
    if (final_cost) HIPCHK(hipMemcpyAsync(final_cost, h->unit_a.p, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MDRP_OK;
}

// The progressive sampler alone, for one table of n records and samples of sample_size records (3, 5, 6 or 7): chunk by chunk through the launch
// the scheduler uses (launch_samples_prosac), the (RNG state, sample index) carried on the device from chunk to chunk.
// out: [sum of chunk_lens][sample_size] uint32 in host memory; n < sample_size writes nothing.
int mdrp_prosac_samples_k(mdrp_handle *h, uint64_t seed, int n, int sample_size, uint64_t max_prosac_iterations, const int32_t *chunk_lens, int n_chunks,
                          uint32_t *out) {
    const char *why = nullptr;
    long long total = 0, longest = 0;
    const int K = sample_size;
    if (!h || n < 0 || n_chunks < 0 || (n_chunks > 0 && (!chunk_lens || !out))) why = "invalid argument";
    else if (K != 3 && K != 5 && K != 6 && K != 7) why = "prosac_samples: sample_size is 3, 5, 6 or 7";
    for (int c = 0; !why && c < n_chunks; ++c) {
        if (chunk_lens[c] < 1) why = "prosac_samples: a chunk length < 1";
        else { total += chunk_lens[c]; longest = std::max<long long>(longest, chunk_lens[c]); }
    }
    if (!why && total > (1 << 24)) why = "prosac_samples: more than 2^24 samples";
    if (why) { g_err = why; return MDRP_ERR_INVALID; }
    if (n < K || n_chunks == 0) return MDRP_OK;
    MDRP_ENTER(h);
    hipStream_t s = h->stream;
    int rc;
    if ((rc = h->params.ensure(16)) || (rc = h->samples[0].ensure(sizeof(uint32_t) * K * (size_t)longest))) return rc;
    uint64_t *d_state = h->params.as<uint64_t>();
    int32_t *d_n = reinterpret_cast<int32_t *>(d_state + 1);
    const int32_t n32 = n;
    HIPCHK(hipMemcpyAsync(d_state, &seed, sizeof seed, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_n, &n32, sizeof n32, hipMemcpyHostToDevice, s));
    ProsacTab tab{nullptr, nullptr, nullptr};
    if ((rc = prosac_tables(h, s, K, &n32, 1, max_prosac_iterations, (uint64_t)total, tab))) return rc;
    const int threads = env_int("MDRP_SAMPLE_THREADS", K == 3 ? SAMP_THREADS : (K == 5 ? 512 : 256)); // (the scheduler's defaults: Pass::samp_threads)
    size_t done = 0;
    for (int c = 0; c < n_chunks; ++c) {
        launch_samples_prosac(s, K, threads, 1, d_n, d_state, tab, max_prosac_iterations, chunk_lens[c], h->samples[0].as<uint32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out + K * done, h->samples[0].p, sizeof(uint32_t) * K * (size_t)chunk_lens[c], hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s)); // (pageable destination: the next chunk overwrites the table)
        done += (size_t)chunk_lens[c];
    }
    return MDRP_OK;
}

int mdrp_prosac_samples(mdrp_handle *h, uint64_t seed, int n, uint64_t max_prosac_iterations, const int32_t *chunk_lens, int n_chunks, uint32_t *out) {
    return mdrp_prosac_samples_k(h, seed, n, 3, max_prosac_iterations, chunk_lens, n_chunks, out);
}

} // extern "C"

// ---- the varying-focal baseline's tail: focals and pose from F (include/mdrp_classic_focals.h; mdrp_classic_focals.h)
namespace {

struct FocalPoseCall {
    const double *x1, *x2;
    int batch, n_max;
    const int32_t *n_per_pair; // host
    const void *models;
    int stride;
    const uint8_t *mask;
    const double *pp1, *pp2;
};

// what the pose entry points refuse before any device work
const char *focal_pose_refusal(const FocalPoseCall &c, const void *out) {
    if (c.batch < 0 || c.n_max < 0) return "focal pose: a negative size";
    if (c.batch > 0 && (!c.models || !out)) return "focal pose: models or out is NULL";
    if (c.batch > 0 && c.n_max > 0 && (!c.x1 || !c.x2)) return "focal pose: correspondences are NULL";
    if (const char *why = n_per_pair_out_of_range(c.n_per_pair, c.batch, c.n_max)) return why;
    if (c.stride < (int)sizeof(mdrp_model) || c.stride % 8 != 0)
        return "focal pose: model_stride_bytes must be a multiple of 8 and at least sizeof(mdrp_model) = 96 (sizeof(mdrp_result) = 136 reads result records)";
    return nullptr;
}

// the counts up, then ONE launch of kc_focal_pose on the handle's stream; every pointer but n_per_pair is device memory
int focal_pose_device(mdrp_handle *h, const FocalPoseCall &c, FocalPose *out_dev) {
    if (c.batch == 0) return MDRP_OK;
    hipStream_t s = h->stream;
    if (int rc = h->fp_nper.ensure(sizeof(int32_t) * (size_t)c.batch)) return rc;
    std::vector<int32_t> nper(c.batch); // pageable: the copy has left it when hipMemcpyAsync returns
    for (int i = 0; i < c.batch; ++i) nper[i] = c.n_per_pair ? c.n_per_pair[i] : c.n_max;
    HIPCHK(hipMemcpyAsync(h->fp_nper.p, nper.data(), sizeof(int32_t) * (size_t)c.batch, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(kc_focal_pose, dim3(c.batch), dim3(FOCAL_POSE_THREADS), 0, s, c.x1, c.x2, c.n_max, (const int32_t *)h->fp_nper.as<int32_t>(),
                       reinterpret_cast<const unsigned char *>(c.models), c.stride, c.mask, c.pp1, c.pp2, out_dev);
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

} // namespace

extern "C" {

int mdrp_focals_from_fundamental(mdrp_handle *h, int mem_space, const double *F, const double *pp1, const double *pp2, int batch, double *f1f2) {
    if (!h || batch < 0 || (batch > 0 && (!F || !f1f2)) || (mem_space != MDRP_MEM_HOST && mem_space != MDRP_MEM_DEVICE)) {
        g_err = "focals: invalid argument";
        return MDRP_ERR_INVALID;
    }
    MDRP_ENTER(h);
    if (batch == 0) return MDRP_OK;
    hipStream_t s = h->stream;
    const size_t b = (size_t)batch;
    const double *dF = F, *d1 = pp1, *d2 = pp2;
    double *dout = f1f2;
    if (mem_space == MDRP_MEM_HOST) {
        const size_t off1 = pad16(sizeof(double) * 9 * b), off2 = off1 + pad16(sizeof(double) * 2 * b);
        int rc;
        if ((rc = h->fp_in.ensure(off2 + sizeof(double) * 2 * b)) || (rc = h->fp_out.ensure(sizeof(double) * 2 * b))) return rc;
        unsigned char *in = h->fp_in.as<unsigned char>();
        HIPCHK(hipMemcpyAsync(in, F, sizeof(double) * 9 * b, hipMemcpyHostToDevice, s));
        if (pp1) HIPCHK(hipMemcpyAsync(in + off1, pp1, sizeof(double) * 2 * b, hipMemcpyHostToDevice, s));
        if (pp2) HIPCHK(hipMemcpyAsync(in + off2, pp2, sizeof(double) * 2 * b, hipMemcpyHostToDevice, s));
        dF = reinterpret_cast<const double *>(in);
        d1 = pp1 ? reinterpret_cast<const double *>(in + off1) : nullptr;
        d2 = pp2 ? reinterpret_cast<const double *>(in + off2) : nullptr;
        dout = h->fp_out.as<double>();
    }
    hipLaunchKernelGGL(kc_focals, dim3((batch + 255) / 256), dim3(256), 0, s, dF, d1, d2, batch, dout);
    HIPCHK(hipGetLastError());
    if (mem_space == MDRP_MEM_HOST) HIPCHK(hipMemcpyAsync(f1f2, dout, sizeof(double) * 2 * b, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MDRP_OK;
}

int mdrp_pose_from_fundamental_async(mdrp_handle *h, const double *x1, const double *x2, int batch, int n_max, const int32_t *n_per_pair, const void *models,
                                     int model_stride_bytes, const uint8_t *inlier_mask, const double *pp1, const double *pp2, mdrp_focal_pose *out_dev) {
    const FocalPoseCall c{x1, x2, batch, n_max, n_per_pair, models, model_stride_bytes, inlier_mask, pp1, pp2};
    const char *why = h ? focal_pose_refusal(c, out_dev) : "focal pose: invalid argument";
    if (why) { g_err = why; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    return focal_pose_device(h, c, reinterpret_cast<FocalPose *>(out_dev));
}

int mdrp_pose_from_fundamental(mdrp_handle *h, int mem_space, const double *x1, const double *x2, int batch, int n_max, const int32_t *n_per_pair,
                               const void *models, int model_stride_bytes, const uint8_t *inlier_mask, const double *pp1, const double *pp2,
                               mdrp_focal_pose *out) {
    FocalPoseCall c{x1, x2, batch, n_max, n_per_pair, models, model_stride_bytes, inlier_mask, pp1, pp2};
    const char *why = h ? focal_pose_refusal(c, out) : "focal pose: invalid argument";
    if (!why && mem_space != MDRP_MEM_HOST && mem_space != MDRP_MEM_DEVICE) why = "focal pose: invalid argument";
    if (why) { g_err = why; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    if (batch == 0) return MDRP_OK;
    hipStream_t s = h->stream;
    const size_t b = (size_t)batch, np = b * (size_t)n_max;
    int rc;
    if ((rc = h->fp_out.ensure(sizeof(FocalPose) * b))) return rc;
    if (mem_space == MDRP_MEM_HOST) { // the inputs in one piece each on the handle's stream, as stage_host_call copies them
        const size_t sz_models = pad16(b * (size_t)model_stride_bytes), sz_mask = pad16(np), sz_pp = pad16(sizeof(double) * 2 * b);
        const size_t off_mask = sz_models, off_pp1 = off_mask + sz_mask, off_pp2 = off_pp1 + sz_pp;
        if ((rc = h->in_x1.ensure(sizeof(double) * 2 * np + 16)) || (rc = h->in_x2.ensure(sizeof(double) * 2 * np + 16)) || (rc = h->fp_in.ensure(off_pp2 + sz_pp)))
            return rc;
        unsigned char *in = h->fp_in.as<unsigned char>();
        if (np > 0) {
            HIPCHK(hipMemcpyAsync(h->in_x1.p, x1, sizeof(double) * 2 * np, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(h->in_x2.p, x2, sizeof(double) * 2 * np, hipMemcpyHostToDevice, s));
        }
        HIPCHK(hipMemcpyAsync(in, models, b * (size_t)model_stride_bytes, hipMemcpyHostToDevice, s));
        if (inlier_mask && np > 0) HIPCHK(hipMemcpyAsync(in + off_mask, inlier_mask, np, hipMemcpyHostToDevice, s));
        if (pp1) HIPCHK(hipMemcpyAsync(in + off_pp1, pp1, sizeof(double) * 2 * b, hipMemcpyHostToDevice, s));
        if (pp2) HIPCHK(hipMemcpyAsync(in + off_pp2, pp2, sizeof(double) * 2 * b, hipMemcpyHostToDevice, s));
        c.x1 = h->in_x1.as<double>(); c.x2 = h->in_x2.as<double>();
        c.models = in;
        c.mask = inlier_mask ? in + off_mask : nullptr;
        c.pp1 = pp1 ? reinterpret_cast<const double *>(in + off_pp1) : nullptr;
        c.pp2 = pp2 ? reinterpret_cast<const double *>(in + off_pp2) : nullptr;
    }
    if ((rc = focal_pose_device(h, c, h->fp_out.as<FocalPose>()))) return rc;
    HIPCHK(hipMemcpyAsync(out, h->fp_out.p, sizeof(FocalPose) * b, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MDRP_OK;
}

int mdrp_estimate_fundamental_focals_async(mdrp_handle *h, const double *x1, const double *x2, int batch, int n_max, const int32_t *n_per_pair,
                                           const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, uint8_t *inlier_mask_dev, const double *pp1,
                                           const double *pp2, mdrp_focal_pose *out_dev) {
    if (!h) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    EstimateCall c = call_of(MDRP_FUNDAMENTAL_7PT, x1, x2, nullptr, nullptr, batch, n_max, n_per_pair, nullptr, nullptr, ropt, bopt);
    c.mask_dev = inlier_mask_dev;
    MDRP_ENTER(h);
    if (int rc = estimate_refusals(h, c)) return rc; // (the estimator's own, first: its option refusals keep their codes)
    const char *why = nullptr;
    if (batch > 0 && !out_dev) why = "focal pose: models or out is NULL";
    else if (batch > 0 && n_max > 0 && (!x1 || !x2)) why = "focal pose: correspondences are NULL";
    else why = n_per_pair_out_of_range(n_per_pair, batch, n_max);
    if (why) { g_err = why; return MDRP_ERR_INVALID; }
    if (int rc = estimate_device(h, c)) return rc;
    if (batch == 0) return MDRP_OK;
    // the tail behind the estimator on the handle's stream: its records and its mask where they lie
    const FocalPoseCall fc{x1, x2, batch, n_max, n_per_pair, h->results.p, (int)sizeof(ResultDev), inlier_mask_dev ? inlier_mask_dev : h->mask.as<uint8_t>(), pp1, pp2};
    return focal_pose_device(h, fc, reinterpret_cast<FocalPose *>(out_dev));
}

} // extern "C"

// ---- the front end for dense matchers: a warp sampled by certainty (include/mdrp_dense.h; mdrp_dense.h)
namespace {

static_assert(MDRP_DENSE_NORMALIZED == DENSE_NORMALIZED && MDRP_DENSE_PIXEL == DENSE_PIXEL && MDRP_DENSE_MAX_ROWS == DENSE_MAX_ROWS &&
              MDRP_DENSE_MAX_STAGE1 == DENSE_MAX_STAGE1 && MDRP_DENSE_MAX_N == DENSE_MAX_N && MDRP_DENSE_MAX_GRID == DENSE_MAX_GRID, "limits of the header and of the kernels");
static_assert(sizeof(mdrp_dense_matches) == 144 && offsetof(mdrp_dense_matches, seed) == 112 && offsetof(mdrp_dense_matches, rows_out) == 128, "descriptor layout");

// what both entry points refuse of the descriptor before any device work
const char *dense_refusal(const mdrp_dense_matches *d, int batch) {
    const auto is_type = [](int t) { return t == MDRP_F32 || t == MDRP_F64; };
    if (!d || batch < 0) return "invalid argument";
    if (!is_type(d->warp_type) || !is_type(d->certainty_type) || !is_type(d->depth_type)) return "warp_type / certainty_type / depth_type must be MDRP_F32 or MDRP_F64";
    if (d->coords != MDRP_DENSE_NORMALIZED && d->coords != MDRP_DENSE_PIXEL) return "coords must be MDRP_DENSE_NORMALIZED or MDRP_DENSE_PIXEL";
    if (d->filter != MDRP_FILTER_BOTH_INF && d->filter != MDRP_FILTER_FINITE) return "unknown filter";
    if (d->rows < 0 || d->h1 < 0 || d->w1 < 0 || d->h2 < 0 || d->w2 < 0) return "negative size";
    if (d->rows > MDRP_DENSE_MAX_ROWS) return "rows above MDRP_DENSE_MAX_ROWS (2^22)";
    if (d->n < 1 || d->n > MDRP_DENSE_MAX_N) return "n must be 1 .. MDRP_DENSE_MAX_N (16384)";
    if (d->expansion < 1) return "expansion must be at least 1";
    if ((int64_t)d->expansion * d->n > MDRP_DENSE_MAX_STAGE1) return "expansion * n above MDRP_DENSE_MAX_STAGE1 (65536)";
    if (d->grid < 1 || d->grid > MDRP_DENSE_MAX_GRID) return "grid must be 1 .. MDRP_DENSE_MAX_GRID (8)";
    if (d->min_count < 1) return "min_count must be at least 1";
    if (batch > 0 && d->rows > 0 && (!d->warp || !d->certainty)) return "NULL warp or certainty";
    if (batch > 0 && ((d->h1 > 0 && d->w1 > 0 && !d->depth1) || (d->h2 > 0 && d->w2 > 0 && !d->depth2))) return "NULL depth map";
    return nullptr;
}
int check_dense(const mdrp_dense_matches *d, int batch) {
    if (const char *why = dense_refusal(d, batch)) { g_err = std::string("mdrp_dense_matches: ") + why; return MDRP_ERR_INVALID; }
    return MDRP_OK;
}

// The kernels of the sampler on the handle's stream; the outputs are device memory, [batch][n]; n_dev: [batch].  The scratch is one buffer of
// the handle, carved for this call's sizes.
int dense_sample_device(mdrp_handle *h, const mdrp_dense_matches *d, int batch, double *x1, double *x2, double *d1, double *d2, int32_t *rows, double *score,
                        int32_t *n_dev) {
    if (batch == 0) return MDRP_OK;
    hipStream_t s = h->stream;
    DenseArgs a{};
    a.warp = d->warp; a.cert = d->certainty; a.depth1 = d->depth1; a.depth2 = d->depth2; a.center1 = d->center1; a.center2 = d->center2;
    a.warp_type = d->warp_type; a.cert_type = d->certainty_type; a.depth_type = d->depth_type; a.coords = d->coords; a.filter = d->filter;
    a.rows = d->rows; a.h1 = d->h1; a.w1 = d->w1; a.h2 = d->h2; a.w2 = d->w2;
    a.n = d->n; a.m1_max = d->balanced ? d->expansion * d->n : d->n; a.grid = d->grid; a.min_count = d->min_count; a.balanced = d->balanced ? 1 : 0;
    a.ranked = d->ranked ? 1 : 0;
    a.seed = (uint32_t)d->seed; a.threshold = d->threshold;
    a.nblk = std::max(1, (d->rows + DENSE_BLOCK_ROWS - 1) / DENSE_BLOCK_ROWS); // (a warp without rows: one empty block)
    a.ntile = (a.m1_max + DENSE_THREADS - 1) / DENSE_THREADS;
    const size_t b = (size_t)batch, slots = (size_t)a.ntile * DENSE_THREADS;
    Carve cv;
    const size_t o_qpre = cv.take(sizeof(uint32_t) * b * std::max(a.rows, 1)), o_bpre = cv.take(sizeof(uint64_t) * b * a.nblk), o_bcnt = cv.take(sizeof(uint32_t) * b * a.nblk),
                 o_meta = cv.take(sizeof(DenseMeta) * b), o_cand = cv.take(sizeof(int32_t) * b * slots), o_tcnt = cv.take(sizeof(int32_t) * b * a.ntile),
                 o_p1 = cv.take(sizeof(int32_t) * b * a.m1_max), o_cell = cv.take(sizeof(int32_t) * b * a.m1_max), o_wpre = cv.take(sizeof(uint64_t) * b * a.m1_max),
                 o_sel = cv.take(sizeof(int32_t) * b * a.n), o_rank = cv.take(sizeof(int32_t) * b * a.n);
    if (int rc = cv.ensure(h->dn_scratch)) return rc;
    DenseScratch z;
    z.qpre = cv.at<uint32_t>(o_qpre); z.bpre = cv.at<uint64_t>(o_bpre); z.bcnt = cv.at<uint32_t>(o_bcnt);
    z.meta = cv.at<DenseMeta>(o_meta); z.cand = cv.at<int32_t>(o_cand); z.tcnt = cv.at<int32_t>(o_tcnt);
    z.p1 = cv.at<int32_t>(o_p1); z.cell = cv.at<int32_t>(o_cell); z.wpre = cv.at<uint64_t>(o_wpre);
    z.sel = cv.at<int32_t>(o_sel); z.rank = cv.at<int32_t>(o_rank);
    hipLaunchKernelGGL(k_dense_weights, dim3(batch, a.nblk), dim3(DENSE_THREADS), 0, s, a, z.qpre, z.bpre, z.bcnt);
    hipLaunchKernelGGL(k_dense_scan, dim3(batch), dim3(DENSE_THREADS), 0, s, a, z.bpre, (const uint32_t *)z.bcnt, z.meta);
    hipLaunchKernelGGL(k_dense_pick, dim3(batch, a.ntile), dim3(DENSE_THREADS), 0, s, a, (const uint32_t *)z.qpre, (const uint64_t *)z.bpre, (const DenseMeta *)z.meta,
                       z.cand, z.tcnt);
    hipLaunchKernelGGL(k_dense_balance, dim3(batch), dim3(DENSE_BAL_THREADS), 0, s, a, (const int32_t *)z.cand, (const int32_t *)z.tcnt, z.p1, z.cell, z.wpre, z.sel, n_dev);
    if (a.ranked)
        hipLaunchKernelGGL(k_dense_rank, dim3(batch, (a.n + DENSE_EMIT_RECORDS - 1) / DENSE_EMIT_RECORDS), dim3(DENSE_THREADS), 0, s, a.cert, a.cert_type, a.rows, a.n,
                           (const int32_t *)z.sel, (const int32_t *)n_dev, z.rank);
    hipLaunchKernelGGL(k_dense_emit, dim3(batch, (a.n + DENSE_THREADS - 1) / DENSE_THREADS), dim3(DENSE_THREADS), 0, s, a, (const int32_t *)z.sel, (const int32_t *)n_dev,
                       (const int32_t *)(a.ranked ? z.rank : nullptr), x1, x2, d1, d2, rows, score);
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

} // namespace

extern "C" {

int mdrp_sample_dense(mdrp_handle *h, const mdrp_dense_matches *desc, int batch, double *x1, double *x2, double *d1, double *d2, int32_t *rows, double *score,
                      int32_t *n_host) {
    if (!h) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (int rc = check_dense(desc, batch)) return rc;
    if (batch > 0 && (!x1 || !x2 || !d1 || !d2 || !rows || !score || !n_host)) { g_err = "mdrp_sample_dense: NULL output"; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    int rc;
    if ((rc = h->fe_n.ensure(sizeof(int32_t) * std::max(batch, 1)))) return rc;
    if ((rc = dense_sample_device(h, desc, batch, x1, x2, d1, d2, rows, score, h->fe_n.as<int32_t>()))) return rc;
    if ((rc = fetch_counts(h, batch))) return rc;
    if (batch > 0) std::memcpy(n_host, h->fe_n_host, sizeof(int32_t) * batch);
    return MDRP_OK;
}

int mdrp_estimate_dense_async(mdrp_handle *h, int kind, const mdrp_dense_matches *desc, int batch, const mdrp_camera *cam1, const mdrp_camera *cam2,
                              const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, uint8_t *record_mask_dev, int32_t *n_used_host) {
    if (!h || !ropt || !bopt) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (int rc = check_front_end_kind(kind, true, "mdrp_estimate_dense_async")) return rc;
    if (int rc = check_dense(desc, batch)) return rc;
    static const double own = 0.0; // the records are buffers of the handle, not yet sized: `own` stands for them in the refusals (as in estimate_front)
    const bool ranked = desc->ranked != 0;
    const int n = desc->n;
    EstimateCall c = call_of(kind, nullptr, nullptr, &own, &own, batch, n, nullptr, cam1, cam2, ropt, bopt);
    if (int rc = refusals_as_run(h, c, ranked)) return rc;
    MDRP_ENTER(h);
    const size_t recs = (size_t)batch * n;
    int rc;
    if ((rc = ensure_gather_buffers(h, batch, n, true)) || (!desc->score_out && (rc = h->dn_score.ensure(sizeof(double) * recs + 16)))) return rc;
    int32_t *rows = desc->rows_out ? desc->rows_out : h->fe_slot.as<int32_t>();
    double *score = desc->score_out ? desc->score_out : h->dn_score.as<double>();
    c.x1 = h->fe_x1.as<double>(); c.x2 = h->fe_x2.as<double>(); c.d1 = h->fe_d1.as<double>(); c.d2 = h->fe_d2.as<double>();
    if ((rc = dense_sample_device(h, desc, batch, h->fe_x1.as<double>(), h->fe_x2.as<double>(), h->fe_d1.as<double>(), h->fe_d2.as<double>(), rows, score,
                                  h->fe_n.as<int32_t>())))
        return rc;
    if ((rc = fetch_counts(h, batch))) return rc;
    c.n_per_pair = batch > 0 ? h->fe_n_host.v : nullptr;
    c.mask_dev = record_mask_dev; // per sampled record, in the records' order: nothing to map back
    const RankedRun rr(*ropt);
    if (ranked) rr.apply(c); // the records are in quality order: the progressive sampler on them as they are
    if ((rc = estimate_device(h, c))) return rc;
    if (n_used_host && batch > 0) std::memcpy(n_used_host, h->fe_n_host, sizeof(int32_t) * batch);
    return MDRP_OK;
}

} // extern "C"

// ---- the back end: fused two-view point clouds from models and depth maps (include/mdrp_reconstruct.h; mdrp_reconstruct.h)
namespace {

static_assert(MDRP_KEEP_NOT_INF == RECON_KEEP_NOT_INF && MDRP_KEEP_FINITE == RECON_KEEP_FINITE && MDRP_RECON_MAX_EXTENT == RECON_MAX_EXTENT &&
              MDRP_RECON_ALL == RECON_ALL && sizeof(mdrp_model) == RECON_MODEL_BYTES, "values of the header and of the kernels");
static_assert(sizeof(mdrp_depth_pairs) == 56 && offsetof(mdrp_depth_pairs, center1) == 40 && sizeof(mdrp_depth_image_pairs) == 48 &&
              offsetof(mdrp_depth_image_pairs, size) == 24 && sizeof(mdrp_reconstruct_opt) == 24 && offsetof(mdrp_reconstruct_opt, p_max) == 16, "descriptor layout");
static_assert(sizeof(ReconCam) == sizeof(mdrp_camera) && offsetof(ReconCam, params) == offsetof(mdrp_camera, params), "camera layout");

// one call of a two-view entry point (clouds or co-visibility): the descriptor and the options flattened (ReconArgs without its tile counts) and
// everything else the caller handed over
struct ReconCall {
    const char *who;
    ReconArgs a;
    int batch;
    const mdrp_camera *cam1, *cam2; // host
    float *points;
    int32_t *pixel, *counts;
};
ReconCall recon_call(const char *who, int kind, int batch, const void *models_dev, int model_stride, const mdrp_camera *cam1, const mdrp_camera *cam2, float *points,
                     int32_t *pixel, int32_t *counts) {
    ReconCall c{who, {}, batch, cam1, cam2, points, pixel, counts};
    c.a.models = static_cast<const unsigned char *>(models_dev); c.a.model_stride = model_stride; c.a.kind = kind;
    return c;
}
// the two descriptors into ReconArgs (struct ReconArgs, mdrp_reconstruct.h)
void recon_flatten(ReconArgs &a, const mdrp_depth_pairs *dp) {
    a.depth1 = dp->depth1; a.depth2 = dp->depth2; a.center1 = dp->center1; a.center2 = dp->center2;
    a.depth_type = dp->depth_type;
    a.h1 = dp->h1; a.w1 = dp->w1; a.h2 = dp->h2; a.w2 = dp->w2;
}
void recon_flatten(ReconArgs &a, const mdrp_depth_image_pairs *ip) {
    a.depth1 = a.depth2 = ip->n_images > 0 ? ip->depth : ip; // (an empty set: no map is read; the pointer only has to pass for one)
    a.center1 = a.center2 = ip->center; a.size = ip->size; a.pairs = ip->pairs; a.n_images = ip->n_images;
    a.depth_type = ip->depth_type;
    a.h1 = a.h2 = ip->h_max; a.w1 = a.w2 = ip->w_max;
}

// The runs of refusals that the back end's entry points share; each entry point composes them in its own order, which decides the message of a call
// with two defects.
const char *recon_kind_refusal(int kind) {
    return kind < MDRP_CALIB || kind > MDRP_VARYING_FOCAL ? "only the monodepth estimators' models (kind 0..2) have depths to unproject" : nullptr;
}
const char *recon_stride_refusal(int model_stride) {
    return model_stride < RECON_MODEL_BYTES || model_stride % 8 != 0 ? "model_stride must be at least 96 and a multiple of 8" : nullptr;
}
const char *recon_focal_cameras_refusal(int kind, bool cameras) {
    return kind != MDRP_CALIB && cameras ? "cameras are MDRP_CALIB's: a focal kind unprojects with the model's focals (pass NULL)" : nullptr;
}
const char *recon_option_refusal(int depth_type, int keep, uint32_t thr, int p_max) {
    if (depth_type != MDRP_F32 && depth_type != MDRP_F64) return "depth_type must be MDRP_F32 or MDRP_F64";
    if (keep != MDRP_KEEP_NOT_INF && keep != MDRP_KEEP_FINITE) return "keep must be MDRP_KEEP_NOT_INF or MDRP_KEEP_FINITE";
    if (thr == 0) return "thr == 0 keeps nothing (1 .. MDRP_RECON_ALL)";
    if (p_max < 0) return "negative p_max";
    return nullptr;
}
const char *recon_extent_refusal(int h1, int w1, int h2, int w2, int n_images) {
    if (h1 < 0 || w1 < 0 || h2 < 0 || w2 < 0 || n_images < 0) return "negative size";
    if (h1 > MDRP_RECON_MAX_EXTENT || w1 > MDRP_RECON_MAX_EXTENT || h2 > MDRP_RECON_MAX_EXTENT || w2 > MDRP_RECON_MAX_EXTENT)
        return "extent above MDRP_RECON_MAX_EXTENT (65536)";
    if ((int64_t)h1 * w1 > INT32_MAX || (int64_t)h2 * w2 > INT32_MAX) return "a map of 2^31 pixels or more";
    return nullptr;
}
const char *recon_camera_models_refusal(const mdrp_camera *cams, int n) {
    for (int i = 0; i < n; ++i)
        if ((cams[i].model_id | 1) != 1) return "only SIMPLE_PINHOLE (0) and PINHOLE (1) cameras unproject here";
    return nullptr;
}

// what the two-view entry points refuse before any device work (the descriptor's own NULLs are the entry points')
const char *recon_refusal(const ReconCall &c) {
    const ReconArgs &a = c.a;
    const char *why;
    if (c.batch < 0) return "negative batch";
    if ((why = recon_kind_refusal(a.kind))) return why;
    if (a.kind == MDRP_CALIB && c.batch > 0 && (!c.cam1 || !c.cam2)) return "MDRP_CALIB needs cam1_host and cam2_host, one record per pair";
    if ((why = recon_focal_cameras_refusal(a.kind, c.cam1 || c.cam2))) return why;
    if ((why = recon_stride_refusal(a.model_stride))) return why;
    if ((why = recon_option_refusal(a.depth_type, a.keep, a.thr, a.p_max))) return why;
    if ((why = recon_extent_refusal(a.h1, a.w1, a.h2, a.w2, a.n_images))) return why;
    if (c.batch == 0) return nullptr;
    if (!a.models || !c.counts) return "NULL models_dev or counts";
    if (a.p_max > 0 && (!c.points || !c.pixel)) return "NULL points or pixel";
    if (((int64_t)a.h1 * a.w1 > 0 && !a.depth1) || ((int64_t)a.h2 * a.w2 > 0 && !a.depth2)) return "NULL depth map";
    if (a.kind == MDRP_CALIB && ((why = recon_camera_models_refusal(c.cam1, c.batch)) || (why = recon_camera_models_refusal(c.cam2, c.batch)))) return why;
    return nullptr;
}

int recon_tiles(int h, int w) { return (int)std::max<int64_t>(1, ((int64_t)h * w + RECON_TILE - 1) / RECON_TILE); } // (a map without pixels: one empty tile)

// the call's tile counts from its extents and p_max; the refusal of a grid it cannot launch (batch >= 0)
const char *recon_tile_counts(ReconCall &c) {
    ReconArgs &a = c.a;
    a.nt1 = recon_tiles(a.h1, a.w1); a.nt2 = recon_tiles(a.h2, a.w2); a.nfill = (a.p_max + RECON_TILE - 1) / RECON_TILE;
    return (size_t)c.batch * ((size_t)a.nt1 + a.nt2 + a.nfill) > (size_t)INT32_MAX ? "batch * tiles above 2^31 - 1: split the batch" : nullptr;
}

// The caller's camera table(s) of `count` records each into a carved block, the second behind the first.  Pageable: the copies have left the caller's
// tables when hipMemcpyAsync returns.
int upload_cameras(mdrp_handle *h, ReconCam *dst, const mdrp_camera *cams1, const mdrp_camera *cams2, size_t count) {
    HIPCHK(hipMemcpyAsync(dst, cams1, sizeof(ReconCam) * count, hipMemcpyHostToDevice, h->stream));
    if (cams2) HIPCHK(hipMemcpyAsync(dst + count, cams2, sizeof(ReconCam) * count, hipMemcpyHostToDevice, h->stream));
    return MDRP_OK;
}
// ... of a calibrated two-view call, per pair
int upload_pair_cameras(mdrp_handle *h, ReconCall &c, ReconCam *dst) {
    if (c.a.kind != MDRP_CALIB) return MDRP_OK;
    c.a.cam1 = dst; c.a.cam2 = dst + c.batch;
    return upload_cameras(h, dst, c.cam1, c.cam2, (size_t)c.batch);
}

// The three kernels on the handle's stream.  The scratch is the back end's buffer of the handle, carved for this call's sizes; every word of it that
// a kernel reads was written by this call.
int reconstruct_device(mdrp_handle *h, ReconCall &c) {
    ReconArgs &a = c.a;
    if (const char *why = recon_tile_counts(c)) { g_err = std::string(c.who) + ": " + why; return MDRP_ERR_INVALID; }
    if (c.batch == 0) return MDRP_OK;
    const size_t b = (size_t)c.batch, nt = (size_t)a.nt1 + a.nt2;
    Carve cv;
    const size_t o_pair = cv.take(sizeof(ReconPair) * b), o_cam = cv.take(sizeof(ReconCam) * 2 * b), o_tcnt = cv.take(sizeof(uint32_t) * b * nt);
    int rc;
    if ((rc = cv.ensure(h->be_scratch)) || (rc = upload_pair_cameras(h, c, cv.at<ReconCam>(o_cam)))) return rc;
    hipStream_t s = h->stream;
    ReconPair *rp = cv.at<ReconPair>(o_pair);
    uint32_t *tcnt = cv.at<uint32_t>(o_tcnt);
    hipLaunchKernelGGL(k_recon_count, dim3((unsigned)(b * nt)), dim3(RECON_THREADS), 0, s, a, tcnt);
    hipLaunchKernelGGL(k_recon_scan, dim3(c.batch), dim3(RECON_THREADS), 0, s, a, tcnt, rp, c.counts);
    if (a.p_max > 0)
        hipLaunchKernelGGL(k_recon_emit, dim3((unsigned)(b * (nt + a.nfill))), dim3(RECON_THREADS), 0, s, a, (const uint32_t *)tcnt, (const ReconPair *)rp,
                           (const int32_t *)c.counts, c.points, c.pixel);
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

int reconstruct_call(mdrp_handle *h, ReconCall &c, const mdrp_reconstruct_opt *o) {
    c.a.keep = o->keep; c.a.thr = o->thr; c.a.seed = (uint32_t)o->seed; c.a.p_max = o->p_max;
    if (const char *why = recon_refusal(c)) { g_err = std::string(c.who) + ": " + why; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    return reconstruct_device(h, c);
}

} // namespace

extern "C" {

int mdrp_reconstruct_pairs_async(mdrp_handle *h, int kind, const mdrp_depth_pairs *dp, const mdrp_reconstruct_opt *opt, int batch, const void *models_dev,
                                 int model_stride, const mdrp_camera *cam1, const mdrp_camera *cam2, float *points, int32_t *pixel, int32_t *counts) {
    if (!h || !dp || !opt) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    ReconCall c = recon_call("mdrp_reconstruct_pairs_async", kind, batch, models_dev, model_stride, cam1, cam2, points, pixel, counts);
    recon_flatten(c.a, dp);
    return reconstruct_call(h, c, opt);
}

int mdrp_reconstruct_image_pairs_async(mdrp_handle *h, int kind, const mdrp_depth_image_pairs *ip, const mdrp_reconstruct_opt *opt, int batch,
                                       const void *models_dev, int model_stride, const mdrp_camera *cam1, const mdrp_camera *cam2, float *points,
                                       int32_t *pixel, int32_t *counts) {
    if (!h || !ip || !opt) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (batch > 0 && !ip->pairs) { g_err = "mdrp_reconstruct_image_pairs_async: NULL pairs"; return MDRP_ERR_INVALID; }
    ReconCall c = recon_call("mdrp_reconstruct_image_pairs_async", kind, batch, models_dev, model_stride, cam1, cam2, points, pixel, counts);
    recon_flatten(c.a, ip);
    return reconstruct_call(h, c, opt);
}

} // extern "C"

// ---- scenes: an image set's pairs chained along a tree, one fused cloud per scene (include/mdrp_scene.h; mdrp_scene.h)
namespace {

static_assert(MDRP_SCENE_ABSENT == SCENE_ABSENT && MDRP_SCENE_EDGE == SCENE_EDGE && MDRP_SCENE_ROOT == SCENE_ROOT, "values of the header and of the kernels");
static_assert(sizeof(mdrp_scene_transform) == 128 && sizeof(SceneTransform) == 128 && offsetof(mdrp_scene_transform, t) == offsetof(SceneTransform, t) &&
              offsetof(mdrp_scene_transform, s) == offsetof(SceneTransform, s) && offsetof(mdrp_scene_transform, f) == offsetof(SceneTransform, f) &&
              offsetof(mdrp_scene_transform, shift) == offsetof(SceneTransform, shift) && offsetof(mdrp_scene_transform, root) == offsetof(SceneTransform, root) &&
              offsetof(mdrp_scene_transform, depth) == offsetof(SceneTransform, depth) && offsetof(mdrp_scene_transform, depth) == 124, "record layout");

// what both entry points refuse of the tree and the models
const char *scene_tree_refusal(const SceneTree &t) {
    if (t.batch < 0) return "negative batch";
    if (t.n_images < 0) return "negative n_images";
    if (const char *why = recon_kind_refusal(t.kind)) return why;
    if (const char *why = recon_stride_refusal(t.model_stride)) return why;
    if (t.n_images > 0 && !t.tree) return "NULL tree_dev";
    if (t.n_images > 0 && t.batch > 0 && (!t.models || !t.pairs)) return "NULL models_dev or pairs";
    return nullptr;
}

void scene_chain_launch(hipStream_t s, const SceneTree &t, const ReconCam *cams, SceneTransform *T, SceneImage *im) {
    hipLaunchKernelGGL(k_scene_chain, dim3((unsigned)((t.n_images + SCENE_CHAIN_THREADS - 1) / SCENE_CHAIN_THREADS)), dim3(SCENE_CHAIN_THREADS), 0, s, t, cams, T, im);
}

// what the consistency filter (include/mdrp_fuse.h) adds to a scene's cloud: its views, its gate and the rows' support
struct FuseCall {
    const int32_t *views; // device, [n_images][n_views]
    int n_views;
    FuseGate gate;
    uint8_t *support;     // device, [p_max][2]
};
const char *fuse_refusal(const FuseCall &f, int n_images, int p_max) {
    if (f.n_views < 0 || f.n_views > FUSE_MAX_VIEWS) return "n_views must be 0 .. MDRP_FUSE_MAX_VIEWS (8)";
    if (f.n_views > 0 && n_images > 0 && !f.views) return "NULL views_dev";
    if (!(std::isfinite(f.gate.lo) && std::isfinite(f.gate.hi) && f.gate.lo >= 0.0 && f.gate.lo <= 1.0 && f.gate.hi >= 1.0))
        return "lo and hi must be finite with 0 <= lo <= 1 <= hi";
    if (f.gate.min_consistent < 0 || f.gate.max_violating < 0) return "negative min_consistent or max_violating";
    if (p_max > 0 && !f.support) return "NULL support";
    return nullptr;
}

// The scene's cloud behind both of its entry points: every refusal, the scratch and the kernels on the handle's stream.  fuse: null for the plain
// cloud; otherwise the count and emit passes are the filter's (k_fuse_count, k_fuse_emit) behind k_fuse_views, between the same chain and scans.
int scene_cloud(mdrp_handle *h, const char *who, int kind, const mdrp_depth_image_pairs *ip, const mdrp_reconstruct_opt &o, int batch, const void *models_dev,
                int model_stride, const int32_t *tree_dev, const mdrp_camera *cams_host, void *transforms_dev, float *points, int32_t *pixel, int64_t *offsets,
                const FuseCall *fuse) {
    const int n = ip->n_images;
    const SceneTree t{static_cast<const unsigned char *>(models_dev), ip->pairs, tree_dev, model_stride, kind, batch, n};
    const int64_t px = (int64_t)ip->h_max * ip->w_max;
    const auto refusal = [&]() -> const char * {
        const char *why;
        if ((why = scene_tree_refusal(t))) return why;
        if (kind == MDRP_CALIB && n > 0 && !cams_host) return "MDRP_CALIB needs cams_host, one record per image";
        if ((why = recon_focal_cameras_refusal(kind, cams_host != nullptr))) return why;
        if ((why = recon_option_refusal(ip->depth_type, o.keep, o.thr, o.p_max))) return why;
        if ((why = recon_extent_refusal(ip->h_max, ip->w_max, ip->h_max, ip->w_max, n))) return why; // (n >= 0: the tree's refusals)
        if (!offsets) return "NULL offsets";
        if (o.p_max > 0 && (!points || !pixel)) return "NULL points or pixel";
        if (n > 0 && px > 0 && !ip->depth) return "NULL depth map";
        if (kind == MDRP_CALIB && (why = recon_camera_models_refusal(cams_host, n))) return why;
        return fuse ? fuse_refusal(*fuse, n, o.p_max) : nullptr;
    };
    if (const char *why = refusal()) { g_err = std::string(who) + ": " + why; return MDRP_ERR_INVALID; }
    SceneArgs a{};
    a.depth = ip->depth; a.center = ip->center; a.size = ip->size; a.depth_type = ip->depth_type; a.keep = o.keep; a.n_images = n;
    a.h = ip->h_max; a.w = ip->w_max; a.thr = o.thr; a.seed = (uint32_t)o.seed; a.p_max = o.p_max;
    a.nt = recon_tiles(a.h, a.w);
    const size_t tiles = (size_t)n * (size_t)a.nt, nfill = ((size_t)a.p_max + RECON_TILE - 1) / RECON_TILE;
    if (tiles + nfill > (size_t)INT32_MAX) { g_err = std::string(who) + ": the scene's tiles above 2^31 - 1: split the scene"; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    // The scratch is the back end's buffer of the handle, carved for this call's sizes (at least 16 bytes: an empty scene still launches on it); every
    // word of it that a kernel reads was written by this call.
    Carve cv;
    const size_t o_T = cv.take(transforms_dev ? 0 : sizeof(SceneTransform) * (size_t)n), o_im = cv.take(sizeof(SceneImage) * (size_t)n),
                 o_cam = cv.take(kind == MDRP_CALIB ? sizeof(ReconCam) * (size_t)n : 0), o_tcnt = cv.take(sizeof(uint32_t) * tiles),
                 o_fv = cv.take(fuse ? sizeof(FuseView) * (size_t)n : 0), o_fr = cv.take(fuse ? sizeof(FuseRow) * (size_t)n : 0);
    if (int rc = cv.ensure(h->be_scratch, 16)) return rc;
    hipStream_t s = h->stream;
    const ReconCam *cams = nullptr;
    if (kind == MDRP_CALIB && n > 0) {
        if (int rc = upload_cameras(h, cv.at<ReconCam>(o_cam), cams_host, nullptr, (size_t)n)) return rc;
        cams = cv.at<ReconCam>(o_cam);
    }
    SceneTransform *T = transforms_dev ? static_cast<SceneTransform *>(transforms_dev) : cv.at<SceneTransform>(o_T);
    SceneImage *im = cv.at<SceneImage>(o_im);
    uint32_t *tcnt = cv.at<uint32_t>(o_tcnt);
    const FuseArgs f{cv.at<FuseView>(o_fv), cv.at<FuseRow>(o_fr), fuse ? fuse->gate : FuseGate{}};
    if (n > 0) {
        scene_chain_launch(s, t, cams, T, im);
        if (fuse) {
            hipLaunchKernelGGL(k_fuse_views, dim3((unsigned)((n + SCENE_CHAIN_THREADS - 1) / SCENE_CHAIN_THREADS)), dim3(SCENE_CHAIN_THREADS), 0, s, a, kind, cams,
                               (const SceneTransform *)T, fuse->views, fuse->n_views, cv.at<FuseView>(o_fv), cv.at<FuseRow>(o_fr));
            hipLaunchKernelGGL(k_fuse_count, dim3((unsigned)tiles), dim3(RECON_THREADS), 0, s, a, f, (const SceneTransform *)T, (const SceneImage *)im, tcnt);
        } else {
            hipLaunchKernelGGL(k_scene_count, dim3((unsigned)tiles), dim3(RECON_THREADS), 0, s, a, (const SceneTransform *)T, tcnt);
        }
        hipLaunchKernelGGL(k_scene_scan, dim3((unsigned)n), dim3(RECON_THREADS), 0, s, 0, n, a.nt, tcnt, offsets);
    }
    hipLaunchKernelGGL(k_scene_scan, dim3(1), dim3(RECON_THREADS), 0, s, 1, n, a.nt, tcnt, offsets);
    if (a.p_max > 0 && fuse)
        hipLaunchKernelGGL(k_fuse_emit, dim3((unsigned)(tiles + nfill)), dim3(RECON_THREADS), 0, s, a, f, (const uint32_t *)tcnt, (const SceneTransform *)T,
                           (const SceneImage *)im, (const int64_t *)offsets, points, pixel, fuse->support);
    else if (a.p_max > 0)
        hipLaunchKernelGGL(k_scene_emit, dim3((unsigned)(tiles + nfill)), dim3(RECON_THREADS), 0, s, a, (const uint32_t *)tcnt, (const SceneTransform *)T,
                           (const SceneImage *)im, (const int64_t *)offsets, points, pixel);
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

} // namespace

extern "C" {

int mdrp_scene_transforms_async(mdrp_handle *h, int kind, int batch, const void *models_dev, int model_stride, const int32_t *pairs_dev, int n_images,
                                const int32_t *tree_dev, mdrp_scene_transform *transforms_dev) {
    if (!h) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    const SceneTree t{static_cast<const unsigned char *>(models_dev), pairs_dev, tree_dev, model_stride, kind, batch, n_images};
    const char *why = scene_tree_refusal(t);
    if (!why && n_images > 0 && !transforms_dev) why = "NULL transforms_dev";
    if (why) { g_err = std::string("mdrp_scene_transforms_async: ") + why; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    if (n_images == 0) return MDRP_OK;
    scene_chain_launch(h->stream, t, nullptr, reinterpret_cast<SceneTransform *>(transforms_dev), nullptr);
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

int mdrp_reconstruct_scene_async(mdrp_handle *h, int kind, const mdrp_depth_image_pairs *ip, const mdrp_reconstruct_opt *opt, int batch, const void *models_dev,
                                 int model_stride, const int32_t *tree_dev, const mdrp_camera *cams_host, mdrp_scene_transform *transforms_dev, float *points,
                                 int32_t *pixel, int64_t *offsets) {
    if (!h || !ip || !opt) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    return scene_cloud(h, "mdrp_reconstruct_scene_async", kind, ip, *opt, batch, models_dev, model_stride, tree_dev, cams_host, transforms_dev, points, pixel,
                       offsets, nullptr);
}

} // extern "C"

// ---- co-visibility: dense depth-consistency counts per pair (include/mdrp_covis.h; mdrp_covis.h)
namespace {

static_assert(MDRP_COVIS_SAMPLED == COVIS_SAMPLED && MDRP_COVIS_FRONT == COVIS_FRONT && MDRP_COVIS_INSIDE == COVIS_INSIDE && MDRP_COVIS_KNOWN == COVIS_KNOWN &&
              MDRP_COVIS_CONSISTENT == COVIS_CONSISTENT && MDRP_COVIS_OCCLUDED == COVIS_OCCLUDED && MDRP_COVIS_VIOLATING == COVIS_VIOLATING &&
              MDRP_COVIS_SLOTS == COVIS_SLOTS, "values of the header and of the kernels");
static_assert(sizeof(mdrp_covis_opt) == 32 && offsetof(mdrp_covis_opt, seed) == 8 && offsetof(mdrp_covis_opt, lo) == 16 && offsetof(mdrp_covis_opt, hi) == 24, "option layout");

// Both entry points behind their descriptors: the two-view back end's refusals on this call's own values (a cloud of no rows that keeps the finite
// depths), the tolerance's, then the two kernels on the handle's stream.  The scratch is the back end's buffer of the handle, carved for this call's
// sizes; every word of it that a kernel reads was written by this call.
int covis_call(mdrp_handle *h, ReconCall &c, const mdrp_covis_opt *o) {
    ReconArgs &a = c.a;
    a.keep = RECON_KEEP_FINITE; a.thr = o->thr; a.seed = (uint32_t)o->seed; a.p_max = 0;
    const char *why = recon_refusal(c);
    if (!why && !(std::isfinite(o->lo) && std::isfinite(o->hi) && o->lo >= 0.0 && o->lo <= 1.0 && o->hi >= 1.0)) why = "lo and hi must be finite with 0 <= lo <= 1 <= hi";
    if (!why) why = recon_tile_counts(c);
    if (why) { g_err = std::string(c.who) + ": " + why; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    if (c.batch == 0) return MDRP_OK;
    const size_t b = (size_t)c.batch, nt = (size_t)a.nt1 + a.nt2;
    Carve cv;
    const size_t o_pair = cv.take(sizeof(CovisPair) * b), o_cam = cv.take(a.kind == MDRP_CALIB ? sizeof(ReconCam) * 2 * b : 0);
    int rc;
    if ((rc = cv.ensure(h->be_scratch)) || (rc = upload_pair_cameras(h, c, cv.at<ReconCam>(o_cam)))) return rc;
    hipStream_t s = h->stream;
    CovisPair *cp = cv.at<CovisPair>(o_pair);
    hipLaunchKernelGGL(k_covis_pair, dim3((unsigned)((b + COVIS_PAIR_THREADS - 1) / COVIS_PAIR_THREADS)), dim3(COVIS_PAIR_THREADS), 0, s, a, c.batch, cp, c.counts);
    hipLaunchKernelGGL(k_covis_count, dim3((unsigned)(b * nt)), dim3(RECON_THREADS), 0, s, a, (const CovisPair *)cp, o->lo, o->hi, c.counts);
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

} // namespace

extern "C" {

int mdrp_covisibility_pairs_async(mdrp_handle *h, int kind, const mdrp_depth_pairs *dp, const mdrp_covis_opt *opt, int batch, const void *models_dev,
                                  int model_stride, const mdrp_camera *cam1, const mdrp_camera *cam2, int32_t *counts) {
    if (!h || !dp || !opt) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    ReconCall c = recon_call("mdrp_covisibility_pairs_async", kind, batch, models_dev, model_stride, cam1, cam2, nullptr, nullptr, counts);
    recon_flatten(c.a, dp);
    return covis_call(h, c, opt);
}

int mdrp_covisibility_image_pairs_async(mdrp_handle *h, int kind, const mdrp_depth_image_pairs *ip, const mdrp_covis_opt *opt, int batch,
                                        const void *models_dev, int model_stride, const mdrp_camera *cam1, const mdrp_camera *cam2, int32_t *counts) {
    if (!h || !ip || !opt) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (batch > 0 && !ip->pairs) { g_err = "mdrp_covisibility_image_pairs_async: NULL pairs"; return MDRP_ERR_INVALID; }
    ReconCall c = recon_call("mdrp_covisibility_image_pairs_async", kind, batch, models_dev, model_stride, cam1, cam2, nullptr, nullptr, counts);
    recon_flatten(c.a, ip);
    return covis_call(h, c, opt);
}

} // extern "C"

// ---- the consistency filter of a scene: only the points that other images' depth maps confirm (include/mdrp_fuse.h; mdrp_fuse.h)
static_assert(MDRP_FUSE_MAX_VIEWS == FUSE_MAX_VIEWS, "values of the header and of the kernels");
static_assert(sizeof(mdrp_fuse_opt) == 48 && offsetof(mdrp_fuse_opt, seed) == 8 && offsetof(mdrp_fuse_opt, p_max) == 16 && offsetof(mdrp_fuse_opt, n_views) == 20 &&
              offsetof(mdrp_fuse_opt, lo) == 24 && offsetof(mdrp_fuse_opt, hi) == 32 && offsetof(mdrp_fuse_opt, min_consistent) == 40 &&
              offsetof(mdrp_fuse_opt, max_violating) == 44, "option layout");

extern "C" {

int mdrp_fuse_scene_async(mdrp_handle *h, int kind, const mdrp_depth_image_pairs *ip, const mdrp_fuse_opt *opt, int batch, const void *models_dev, int model_stride,
                          const int32_t *tree_dev, const int32_t *views_dev, const mdrp_camera *cams_host, void *transforms_dev, float *points, int32_t *pixel,
                          uint8_t *support, int64_t *offsets) {
    if (!h || !ip || !opt) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    const mdrp_reconstruct_opt o{opt->keep, opt->thr, opt->seed, opt->p_max, 0};
    const FuseCall f{views_dev, opt->n_views, {opt->lo, opt->hi, opt->min_consistent, opt->max_violating}, support};
    return scene_cloud(h, "mdrp_fuse_scene_async", kind, ip, o, batch, models_dev, model_stride, tree_dev, cams_host, transforms_dev, points, pixel, offsets, &f);
}

} // extern "C"
