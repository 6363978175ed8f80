/* mdrp.h — C ABI of the MI355X-native RePoseD RANSAC hot path (libmdrp_hip.so).
 *
 * Drop-in boundary.  The reference reaches this path through pybind11
 * (wheel poselib/_core.pyi:446-501) into PoseLib's C++:
 *     estimate_monodepth_relative_pose                @0x224170   (README.md:86, make_pair.py:111, make_video.py:284)
 *     estimate_shared_focal_monodepth_relative_pose   @0x223300   (README.md:90)
 *     estimate_varying_focal_monodepth_relative_pose  @0x223a40   (README.md:96)
 * one image pair per call.  The entry points below bind the same three estimators, batched: B image pairs per
 * call, each pair an independent unit (that is how the reference itself parallelises, eval.py:355-359).
 * mdrp_amd/_capi.py is the ctypes binding; INTEGRATION.md shows the stub a PoseLib maintainer would add.
 *
 * Conventions: plain pointers + sizes, caller owns every buffer, the library never frees caller memory,
 * int return codes (0 = ok), no exceptions cross the boundary.  One HIP stream per handle.  Threading (the reference
 * releases the GIL around its estimators, wrapper @0x8ad01, and is re-entrant): calls on DIFFERENT handles run
 * concurrently from different host threads; calls on the SAME handle are serialised by a lock inside the handle.
 * Every entry point runs on the handle's device and restores the caller's current HIP device before it returns.
 */
#ifndef MDRP_H
#define MDRP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MDRP_CALIB = 0, MDRP_SHARED_FOCAL = 1, MDRP_VARYING_FOCAL = 2,
       /* non-monodepth baselines of the same binary on the same kernels (d1 = d2 = NULL):
        * estimate_relative_pose (wheel _core.pyi:504-529; 5-point, cameras as for MDRP_CALIB; model: q, t) and
        * estimate_fundamental (_core.pyi:309-323; 7-point; model: F row-major in the first nine doubles of mdrp_model). */
       MDRP_RELPOSE_5PT = 3, MDRP_FUNDAMENTAL_7PT = 5,
       /* estimate_shared_focal_relative_pose (wheel _core.pyi: 6-point, one unknown focal length shared by both images;
        * /root/reference/eval_shared_f.py:161).  Pixels relative to nothing: the principal point travels in cam1[i].params[0..1]
        * (cam2 is not read and may be NULL); model: q, t, f1 = f2 = f in pixels */
       MDRP_SHARED_6PT = 4 };

enum { /* return codes */
    MDRP_OK = 0,
    MDRP_ERR_INVALID = 1,   /* bad argument */
    MDRP_ERR_HIP = 2,       /* a HIP runtime call failed; mdrp_last_error() has the text */
    MDRP_ERR_NO_DEVICE = 3, /* no usable gfx950 device */
    MDRP_ERR_UNSUPPORTED = 4 /* ABI 0.4: a RansacOptions switch of the reference that selects behaviour this library does not build
                              * (progressive_sampling = PROSAC; real_focal_check on the 6- / 7-point baselines).  Refused, never ignored:
                              * the reference would switch samplers / drop models and return different results. */
};

enum { /* where the caller's buffers live */
    MDRP_MEM_HOST = 0,
    MDRP_MEM_DEVICE = 1
};

/* MonoDepthTwoViewGeometry + the two focals of MonoDepthImagePair (wheel _core.pyi:134-204):
 * q = (w,x,y,z);  R (d1+shift1) K1^-1 x1 + t = scale (d2+shift2) K2^-1 x2 */
typedef struct {
    double q[4];
    double t[3];
    double scale, shift1, shift2;
    double f1, f2; /* 1.0 for the calibrated estimator */
} mdrp_model;

/* RansacOptions (wheel METADATA:72-91; defaults as the pybind wrapper @0x8ab59-0x8ac44) */
typedef struct {
    uint64_t max_iterations;   /* 100000 */
    uint64_t min_iterations;   /* 1000 */
    double dyn_num_trials_mult; /* 3.0 */
    double success_prob;        /* 0.9999 */
    double max_reproj_error;    /* 12.0 (pixels) */
    double max_epipolar_error;  /* 1.0 (pixels) */
    uint64_t seed;              /* 0 */
    int32_t monodepth_estimate_shift; /* calibrated estimator only; ignored elsewhere exactly like the reference */
    float monodepth_weight_sampson;   /* 1.0.  A float in the reference too (+0x4c); the wrappers hand max(ws, 0) on.  Away from 1 the reference's
                                       * refiners are not self-consistent and the library reproduces them as they are: the Sampson term enters
                                       * the LM COST as ws rho(r^2) but the normal equations as ws^2 w(.) J'J, with w evaluated at r^2 in the
                                       * calibrated refiner and at ws r^2 in the two focal ones (tests/golden/refine_ws.npz). */
    int32_t score_initial_model;      /* 0.  RansacOptions +0x49, set by the binding when an initial pose is passed with it.  What the
                                       * reference then scores first is NOT the caller's pose: ransac_*_relpose reset it to the identity
                                       * (black-box: any initial pose gives the same result).  The reset model has E = 0: no inliers,
                                       * score N eps^2; its LO changes nothing.  Reproduced as that state: records start at
                                       * (0, N eps^2) and `refinements` at 1 (tests/golden/initial.npz). */
    /* ---- ABI 0.4: the remaining RansacOptions fields of the reference (+0x38 progressive_sampling,
     * +0x40 max_prosac_iterations, +0x48 real_focal_check), so that a host can hand its options over unabridged.
     * PROSAC (RandomSampler::initialize_prosac @0x4f8a20) needs the records in quality order, so it is built behind entry points of its own
     * that take the scores: mdrp_estimate_batch_ranked / _async, below.  Every other estimator entry point refuses a non-zero value
     * with MDRP_ERR_UNSUPPORTED, as before.  (This field sits where ABI 0.3 had a zero `reserved_` word.) */
    int32_t progressive_sampling;    /* 0 */
    uint64_t max_prosac_iterations;  /* 100000; read by the ranked entry points only */
    int32_t real_focal_check;        /* 0.  Only the 6- / 7-point baselines look at it in the reference; refused there when set */
    int32_t reserved_;
} mdrp_ransac_opt;

/* BundleOptions (wheel METADATA:94-106) */
typedef struct {
    uint64_t max_iterations; /* 100 */
    int32_t loss_type;       /* 0 TRIVIAL 1 TRUNCATED 2 HUBER 3 CAUCHY 4 TRUNCATED_CAUCHY 5 TRUNCATED_LE_ZACH */
    double loss_scale;       /* 1.0.  Final refinement of the shared- / varying-focal estimators and of the 5- / 6- / 7-point baselines: divided by the
                              * normalisation scale.  The calibrated monodepth estimator IGNORES it, as the reference does
                              * (estimate_monodepth_relative_pose @0x224704): its final loss scale is half the normalised epipolar threshold,
                              * (1/f1 + 1/f2) * max_epipolar_error / 4 — the same number as loss_scale = 1 at max_epipolar_error = 2, the
                              * reference's own setting (tests/golden/options_ref.npz). */
    double gradient_tol;     /* 1e-10 */
    double step_tol;         /* 1e-8 */
    double initial_lambda;   /* 1e-3 */
    double min_lambda;       /* 1e-10 */
    double max_lambda;       /* 1e10 */
} mdrp_bundle_opt;

/* Pinhole intrinsics of one image (Camera, _core.pyi:76-132; only the models the reference callers use):
 * model_id 0 SIMPLE_PINHOLE params {f,cx,cy,-} ; 1 PINHOLE params {fx,fy,cx,cy} */
typedef struct {
    int32_t model_id;
    int32_t pad_;
    double params[4];
} mdrp_camera;

/* One record per image pair: the estimator's return value + RansacStats.  As in the reference, the model of MDRP_CALIB without the shift flag can be a
 * NaN pose (num_inliers 0, model_score N * eps^2) when no sample of the run gave a real pose: the reference's p3p() emits NaN poses for ~3 % of the
 * samples, and such a model is the record until a real one is scored. */
typedef struct {
    mdrp_model model;
    uint64_t refinements, iterations, num_inliers;
    double inlier_ratio, model_score;
} mdrp_result;

typedef struct mdrp_handle mdrp_handle;

/* Library/handle management.  device = HIP device ordinal.  stream = a hipStream_t created by the caller or NULL to
 * let the handle create its own (non-blocking) stream.
 * mdrp_create / mdrp_create_on_stream are MACROS over the exported mdrp_create_ / mdrp_create_on_stream_ (the zlib deflateInit pattern): they hand the
 * ABI version and the size of mdrp_ransac_opt of the header the HOST was compiled against to the library, which refuses a mismatch
 * (MDRP_ERR_INVALID, mdrp_last_error() names both versions) instead of reading option fields past the end of a smaller struct.  A host built
 * against ABI 0.4 or older, which imported the plain symbols, no longer loads against this library: it must be recompiled. */
int mdrp_create_(int device, void *stream, mdrp_handle **out, int abi_version, int ransac_opt_bytes);
/* Same, but `stream` is used exactly as given: NULL means the device's legacy default (null) stream — which is what
 * torch.cuda.current_stream().cuda_stream is (0) unless the caller switched streams.  Work of the handle is then
 * ordered with everything else queued on that stream (inputs produced by earlier kernels, consumers of the mask). */
int mdrp_create_on_stream_(int device, void *stream, mdrp_handle **out, int abi_version, int ransac_opt_bytes);
#define mdrp_create(device, stream, out) mdrp_create_((device), (stream), (out), MDRP_ABI_VERSION, (int)sizeof(mdrp_ransac_opt))
#define mdrp_create_on_stream(device, stream, out) mdrp_create_on_stream_((device), (stream), (out), MDRP_ABI_VERSION, (int)sizeof(mdrp_ransac_opt))
void mdrp_destroy(mdrp_handle *h);
const char *mdrp_last_error(void);
/* "mdrp-hip <ver> (gfx950) MDRP_SRC_HASH=<16 hex digits>": the hash covers mdrp_capi.hip, mdrp_kernels.h, mdrp_math.h,
 * mdrp_classic.h, mdrp_classic_math.h, mdrp_frontend.h, mdrp_schedule.h, mdrp_from_model.h and this header as they were when the library was built (mdrp_amd/build.py source_hash()) */
const char *mdrp_version(void);
/* (major << 16) | minor of the structs and entry points in this header = 0x00000006.  mdrp_ransac_opt grew from 72 to 88 bytes in
 * 0.4; 0.5 made the version check involuntary: handles are created through mdrp_create_ / mdrp_create_on_stream_, which take the host's
 * MDRP_ABI_VERSION and sizeof(mdrp_ransac_opt) (the macros above pass them) and refuse another ABI.  0.6 adds the device front end at the
 * end of this header (the mdrp_matches descriptor and its two entry points); no existing struct or entry point changed. */
#define MDRP_ABI_VERSION 0x00000006
int mdrp_abi_version(void);
/* HIP_VERSION (major * 10^7 + minor * 10^5 + patch) of the toolchain the library was compiled with.  The library carries no HIP
 * runtime of its own (it binds to the host process's libamdhip64 when it is loaded): a host compares this with
 * hipRuntimeGetVersion() of the runtime it links; mdrp_amd/_capi.py refuses a different major. */
int mdrp_hip_build_version(void);
/* block the calling thread until all work queued on the handle's stream is done */
int mdrp_synchronize(mdrp_handle *h);

/* The handle's history.  A handle keeps its scratch buffers (they only grow and are never cleared), the first-chunk length it learnt from its last
 * call (mdrp_stats::first_chunk) and the fused tail's back-off (mdrp_stats::fuse_*_timeouts) from one call to the next.  All of it may change how the
 * next call is SCHEDULED and none of it what the call RETURNS: every entry point below defines its outputs from its own arguments alone, bit for bit,
 * whatever the handle ran before — another estimator, a larger or smaller batch, a call under other MDRP_* schedule settings, a refused call
 * (tests/test_gpu_history.py).
 * Calls on one handle may follow each other without mdrp_synchronize or a fetch in between, the *_async ones included: a call queues its work behind
 * the previous call's on the handle's stream and stages its per-call parameters in memory the previous call has finished reading.  What the earlier
 * call wrote into CALLER-owned device buffers (inlier masks, initial_score / initial_inliers) is complete once the stream has drained; its result
 * records live in the handle and are replaced by the later call's — fetch or copy them first if they are wanted. */

/* Batched estimators.  x1,x2: [B][n_max][2] pixel coordinates; d1,d2: [B][n_max] depths; n_per_pair: [B] valid
 * correspondences per pair (host memory always; NULL = all n_max).  cam1/cam2: [B] cameras (host memory; calibrated
 * estimator only — the focal estimators take principal-point-centred pixels, README.md:88-96).  out: [B] results
 * (host memory).  inlier_mask: [B][n_max] bytes or NULL (same memory space as the inputs).
 * Pairs with fewer than 3 correspondences return zeroed stats with model_score = DBL_MAX and the identity model,
 * like ransac<> @0x22f087.  The call is synchronous with respect to `out`. */
int mdrp_estimate_batch(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, const double *d1,
                        const double *d2, int batch, int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1,
                        const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                        mdrp_result *out, uint8_t *inlier_mask);

/* Same work on buffers that already live on the device, and nothing is copied back: results stay in the handle's device
 * buffers until mdrp_fetch_results / mdrp_copy_results_device.  Used by bench.py so that the timed region holds device work
 * only (inputs resident in HBM).  "async" is relative to the RESULTS, not to the host: the call queues every kernel of a
 * super-chunk without waiting, but the LO-RANSAC stop rule needs one 48-byte progress record per super-chunk on the host
 * (one short hipStreamSynchronize each; a single one when max_iterations == min_iterations). */
int mdrp_estimate_batch_async(mdrp_handle *h, int kind, const double *x1_dev, const double *x2_dev, const double *d1_dev,
                              const double *d2_dev, int batch, int n_max, const int32_t *n_per_pair_host,
                              const mdrp_camera *cam1_host, const mdrp_camera *cam2_host, const mdrp_ransac_opt *ropt,
                              const mdrp_bundle_opt *bopt, uint8_t *inlier_mask_dev);
int mdrp_fetch_results(mdrp_handle *h, mdrp_result *out_host, int batch);
/* The same records into DEVICE memory (e.g. a torch tensor that goes straight into the RCCL all-gather of the poses,
 * SURVEY.md 8e) — nothing crosses PCIe.  Returns after the handle's stream has drained. */
int mdrp_copy_results_device(mdrp_handle *h, void *dst_dev, int batch);

/* ---- unit-parity entry points (the reference exposes the same pieces: _core.pyi:614-619, 871-876, 914-919) ---- */
/* Minimal solvers on `count` independent 3-point problems (host memory).  x1h,x2h: [count][3][3] homogeneous points
 * (z = 1), d1,d2: [count][3].  out: [count][4] models, n_out: [count] number of valid models.
 * solver: 0 calibrated P3P path (shift off), 1 calibrated with shifts, 2 shared focal, 3 varying focal. */
int mdrp_solver_batch(mdrp_handle *h, int solver, const double *x1h, const double *x2h, const double *d1,
                      const double *d2, int count, mdrp_model *out, int32_t *n_out);

/* Inspection, no kernel runs: how many one-wavefront workgroups of the minimal solver (`solver` as above) the runtime's occupancy query places on
 * a compute unit of `device` when each reserves the dynamic LDS the scheduler's rule grants for `resident_per_simd` solver wavefronts per SIMD with
 * `keep_free_bytes` of the unit's LDS left out of their reach (sched::solver_reservation).  reserve_bytes = 0: the rule grants no cap
 * and workgroups_per_cu is what registers alone allow. */
int mdrp_solver_residency(int device, int solver, int resident_per_simd, uint64_t keep_free_bytes, uint64_t *lds_per_cu,
                          uint64_t *reserve_bytes, int *workgroups_per_cu);

/* The baselines' minimal solvers (relpose_5pt @0x14ae80, relpose_7pt @0x4ff2e0) on `count` independent problems, host memory.
 * x1h, x2h: [count][K][3] unit bearings, K = 5 / 7.  out: [count][M] models, M = 10 / 3 (solutions in the reference's order);
 * n_out: [count]. */
int mdrp_classic_solver_batch(mdrp_handle *h, int kind, const double *x1h, const double *x2h, int count, mdrp_model *out,
                              int32_t *n_out);

/* Sampson/MSAC sweep only (compute_sampson_msac_score @0x4f61d0 / @0x4f65d0): `num_models` models against the n
 * normalised correspondences of ONE pair.  kind selects pose scoring with cheirality (MDRP_CALIB, MDRP_RELPOSE_5PT), F built
 * from pose and focals (focal estimators), or the raw F of MDRP_FUNDAMENTAL_7PT models.
 * All pointers in `mem_space`.  scores: [num_models], counts: [num_models]. */
int mdrp_score_models(mdrp_handle *h, int kind, int mem_space, const mdrp_model *models, int num_models,
                      const double *x1, const double *x2, int n, double sq_threshold, double *scores, int32_t *counts);

/* Candidate counts of the MFMA pre-pass alone (k_count): for every model an UPPER bound on its inlier count against the n
 * normalised correspondences of one pair — the number of correspondences the conservative bf16-split filter cannot prove
 * to be outliers.  Host memory.  candidates: [num_models]. */
int mdrp_count_candidates(mdrp_handle *h, int kind, const mdrp_model *models, int num_models, const double *x1,
                          const double *x2, int n, double sq_threshold, int32_t *candidates);

/* The fp32 stage between the two (k_bound) alone: for every model a LOWER bound of its MSAC score and an UPPER bound of its
 * inlier count against the n normalised correspondences of one pair, from packed-fp32 arithmetic with explicit error terms
 * (DESIGN.md 4).  A hypothesis is retired without the exact fp64 sweep when these two bounds prove that it cannot break a
 * record — the tests assert score_lb <= exact score and count_ub >= exact count on adversarial inputs.  A model whose
 * coefficients leave the fp32 range proves nothing: it reports (0, n).  Host memory.  score_lb, count_ub: [num_models]. */
int mdrp_bound_models(mdrp_handle *h, int kind, const mdrp_model *models, int num_models, const double *x1, const double *x2,
                      int n, double sq_threshold, double *score_lb, int32_t *count_ub);

/* The three retirement stages ARMED, as the scheduler strings them together for a chunk behind the run's first, on ONE pair (within ABI
 * 0.6): k_count (one launch, or phase A + phase B) -> k_bound (optional) -> sort -> plan -> one of the three exact sweeps, against the
 * records (rec_cnt, rec_score) written into the pair's state as best_min_cnt / best_min_score.  rec_score >= DBL_MAX: no record (nothing may
 * be retired).  cand_stat_in[2]: the pair's candidate statistics (candidates, evaluations) from which a two-phase count takes its split
 * point; {0, 0}: the pair is never split.  Host memory.
 *   scores, counts [num_models]  the slots: a model the stages retired keeps count -2 (and score DBL_MAX)
 *   left_at [num_models]         1 retired by k_count, 2 retired by k_bound, 3 reached the exact sweep (which may still bail out: count -2)
 *   info [3]                     hypotheses phase A left undecided | survivors of the count | survivors of the bound (= of the count without it)
 *   cand_stat_out [2]            the statistics after the run (a count without records adds its candidates and evaluations to them)
 * tests/test_gpu_retirement.py pins every decision to the record test on the unarmed stages' own numbers. */
#define MDRP_RETIRE_TWO_PHASE 1   /* count: phase A over the leading tiles + phase B over the undecided (else one armed launch that sweeps every tile) */
#define MDRP_RETIRE_BOUND 2       /* run k_bound between the count and the exact sweep */
#define MDRP_RETIRE_SWEEP_SCORE 0 /* exact sweep: k_score (a lane per hypothesis) */
#define MDRP_RETIRE_SWEEP_SPLIT 4 /*   k_score_split (records split over the workgroup) */
#define MDRP_RETIRE_SWEEP_WAVE 8  /*   k_score_w (a wavefront per hypothesis) */
int mdrp_retire_models(mdrp_handle *h, int kind, const mdrp_model *models, int num_models, const double *x1, const double *x2,
                       int n, double sq_threshold, uint64_t rec_cnt, double rec_score, const uint64_t *cand_stat_in, int flags,
                       double *scores, int32_t *counts, int32_t *left_at, int32_t *info, uint64_t *cand_stat_out);

/* The bookkeeping train of ONE super-chunk on caller-given slot tables (within ABI 0.6): what the scheduler issues behind the exact sweeps, launch
 * for launch and with its buffer roles — one k_scan per chunk (the instantiation chosen by the scheduler's own rule from mps and the chunk's
 * length; chunk_off and chunk_len from chunk_lens), k_lo_plan, then k_walk, or k_walk_ckpt when budgets are given.  Nothing is solved, scored or
 * refined: k_lo does not run.  Between k_lo_plan and the walk the triggers are read back, and each one's LO result (ref_score, ref_cnt, refined) is
 * filled from the three lo_* tables at the trigger's slot iter * mps + k_ref: "the LO result of the minimal model in this slot".
 * `batch` pairs start from `states` (the bookkeeping fields of a pair's state; every other field is zero) and end in them: feeding the states —
 * and, with budgets, the checkpoints — of one call into the next with chunk_start advanced by super_len runs several super-chunks.
 * super_len = the sum of chunk_lens; slots per pair = super_len * mps; the trigger list of a pair holds super_len entries (trig_cap).
 * Slot counts: >= 0 a model's inlier count, -1 an empty slot, -2 "no record" (a retired hypothesis), -3 in slot 0 of an iteration the NaN model
 * of the reference's P3P: (0 inliers, n * sq_thr).  Scores of slots with a negative count are not read as records.
 * Host memory throughout.  MDRP_ERR_INVALID: mps other than 4, 12, 16; sample_sz other than 3, 5, 7; batch < 1; no chunk, more than 8, a chunk
 * length < 1 or more than 2^20 iterations in all; budgets that are not >= 1, strictly increasing, at most MDRP_MAX_BUDGETS and at most
 * ropt->max_iterations; a NULL buffer; a trigger that names a slot outside the tables.  Of ropt only max_iterations, min_iterations,
 * dyn_num_trials_mult and success_prob are read.  tests/test_gpu_replay.py pins the train to the sequential loop. */
typedef struct {
    int32_t n, active;
    double sq_thr;
    uint64_t best_min_cnt;
    double best_min_score;
    uint64_t dyn_max_iter, iterations, refinements, num_inliers;
    double inlier_ratio, model_score;
    mdrp_model best;
} mdrp_replay_state;
typedef struct {
    uint32_t iter;    /* iteration inside the super-chunk */
    int32_t k_ref;    /* slot the LO refines: the last record breaker of the iteration */
    int32_t k_min;    /* slot that set a new best minimal score in the iteration, or -1 */
    int32_t cnt_min;
    double score_min;
    int32_t cnt_ref;
    int32_t pad_;
} mdrp_replay_trigger;
typedef struct {
    /* in */
    int32_t mps, sample_sz, batch, n_chunks;
    uint64_t chunk_start;            /* absolute iteration of the super-chunk's first iteration */
    const int32_t *chunk_lens;       /* [n_chunks] */
    const double *slot_score;        /* [batch][super_len * mps] */
    const int32_t *slot_inl;
    const mdrp_model *models;
    const double *lo_score;          /* the LO tables, same shape */
    const int32_t *lo_cnt;
    const mdrp_model *lo_models;
    const uint64_t *budgets;         /* [n_budgets] or NULL */
    int32_t n_budgets, pad_;
    /* in and out */
    mdrp_replay_state *states;       /* [batch] */
    mdrp_replay_state *checkpoints;  /* [n_budgets][batch] (budgets only): budgets <= chunk_start keep what an earlier call wrote */
    /* out */
    mdrp_replay_trigger *triggers;   /* [batch][super_len]: pair p's first n_triggers[n_chunks - 1][p] entries, in iteration order */
    int32_t *n_triggers;             /* [n_chunks][batch]: after each chunk's scan */
    uint64_t *scan_cnt;              /* [n_chunks][batch]: best_min_cnt after each chunk's scan */
    double *scan_score;              /* [n_chunks][batch]: best_min_score after each chunk's scan */
    int32_t *scan_inst;              /* [n_chunks]: 10 * MPS + IPL of the k_scan instantiation launched */
    int32_t *lo_plan;                /* [3 * batch + 2]: prefix[batch + 1] | begin[batch] | end[batch] | total */
    int32_t *n_active;               /* [1] pairs still iterating */
    uint64_t *max_needed;            /* [1] most iterations any of them still certainly needs */
} mdrp_replay;
int mdrp_replay_slots(mdrp_handle *h, const mdrp_ransac_opt *ropt, mdrp_replay *io);

/* The pick and the filter of a run's first chunk on caller-given lists (within ABI 0.6): k_first_pick, then k_first_filter, one workgroup per pair,
 * with the scheduler's buffer roles and strides and nothing solved or scored between them — the caller's slot tables stand in for k_first_score.
 * Four slots per iteration (the 3-point estimators): a hypothesis in slot s belongs to iteration s / 4.
 * A pair's survivor list holds count tags  slot | key << 24  (k_count's candidate density key, read as min(key, 64)), every slot at most once.
 *   pick    the `pick` hypotheses with the highest key, ties by the lowest slot, and the list's lowest slot go on the picked list P (at most
 *           pick + 1 entries); every other one on the rest list.  Both keep the tags.
 *   filter  a hypothesis of the rest list is retired when the records of P's entries at STRICTLY EARLIER iterations — (max count, min score) over
 *           slot_inl / slot_score at the picked slots with a count >= 0 — rule it out with cand = (key * n) >> 6:
 *           cand <= rec_cnt  and  sq_thr (n - cand) >= rec_score (1 + 1e-12).  The others go on the kept list.  evals: += |P| * n per active pair.
 * Lists are filled through atomics: their order is not defined.  A pair with active == 0 leaves every output as the caller initialised it.
 * Host memory throughout.  MDRP_ERR_INVALID, before any device work: batch < 1; slots < 4, no multiple of 4 or above 2^24; pick outside 1..64; a
 * NULL buffer; a negative n; a list longer than the table; a tag whose slot is outside the table.  tests/test_gpu_first_front.py pins both kernels
 * to the restatement in tests/first_front_ref.py. */
typedef struct {
    /* in */
    int32_t batch, slots;            /* pairs; slots per pair (4 per iteration) */
    int32_t pick, pad_;
    const int32_t *n;                /* [batch] correspondences */
    const int32_t *active;           /* [batch] */
    const double *sq_thr;            /* [batch] */
    const int32_t *count;            /* [batch] length of the survivor list */
    const uint32_t *tags;            /* [batch][slots]: the pair's first count[p] entries */
    const double *slot_score;        /* [batch][slots]: read at the picked slots only */
    const int32_t *slot_inl;
    /* in and out */
    uint32_t *tags_pick;             /* [batch][slots]: the first pick_count[p] entries */
    uint32_t *tags_rest;             /* [batch][slots]: the first rest_count[2 p] entries */
    uint32_t *tags_out;              /* [batch][slots]: the kept list, surv_count[p] entries */
    int32_t *pick_count;             /* [batch] */
    int32_t *rest_count;             /* [2 batch]: pair p's at 2 p; the odd entries are not touched */
    int32_t *surv_count;             /* [batch] */
    /* out */
    uint64_t *evals;                 /* [1] */
} mdrp_front_tables;
int mdrp_front_lists(mdrp_handle *h, mdrp_front_tables *io);

/* The train of a run's FIRST chunk on ONE pair with caller-given models (within ABI 0.6), as the scheduler strings it together for the 3-point
 * estimators in calls of more than 128 pairs: k_count in one launch — without records, or against (rec_cnt, rec_score) the way a prior arms it;
 * rec_score >= DBL_MAX: no record — then the prefix retirement through the function the estimator launches it with (k_first_pick, sort, plan,
 * k_first_score, k_first_filter), then sort, plan and k_score on what is left.  Models in slot order, four per iteration.  A model with a NaN in q
 * or t is what the solver's NaN model is: slot count -3, on no list.  kind: MDRP_CALIB, MDRP_SHARED_FOCAL or MDRP_VARYING_FOCAL; pick in 1..64.
 *   scores, counts [num_models]  the slots: a retired model keeps count -2 (and score DBL_MAX)
 *   left_at [num_models]         0 on no list (a NaN model), 1 retired by k_count, 4 picked (scored by k_first_score), 5 retired by
 *                                k_first_filter, 3 kept by it and scored by k_score
 *   info [5]                     survivors of the count | entries of P | of the rest list | of the kept list | hypotheses k_first_filter
 *                                reports as evaluated (its evals increment / n)
 * Host memory.  tests/test_gpu_first_front.py. */
int mdrp_front_models(mdrp_handle *h, int kind, const mdrp_model *models, int num_models, const double *x1, const double *x2, int n,
                      double sq_threshold, uint64_t rec_cnt, double rec_score, int pick, double *scores, int32_t *counts, int32_t *left_at,
                      int32_t *info);

/* The stages IN FRONT of the sweeps, as the scheduler runs them for a batch (within ABI 0.6: a new symbol only): plan and scratch of one pass, the
 * per-call parameters, k_prep / kc_prep, then for each chunk of the caller's list, in order, the sample tables (the first two drawn ahead beside the
 * prep where the super-chunk is pipelined, as in an estimate) and the minimal solver of the whole batch — through the functions an estimate calls,
 * and nothing behind the solver.  One super-chunk at iteration 0; MDRP_SAMPLE_THREADS, MDRP_SOLVE_RESIDENT, MDRP_LO_OVERLAP and MDRP_CHUNKS (which only
 * sizes the 5-point solver's first-chunk scratch here) act as on an estimate.
 * Before the first launch the records, the fragments, the slot tables, both sample tables and both tag lists are filled with the byte MDRP_FRONT_FILL; the sample table and tag
 * list of a chunk that is not drawn ahead are filled again in front of it.  What no kernel writes keeps the pattern.
 *   kind 0..5, cameras, depths and options as mdrp_estimate_batch takes them (host memory); ropt->monodepth_estimate_shift selects the shift solver
 *   chunk_lens [n_chunks]   1 to 8 chunks of >= 1 iterations; super_len = their sum; chunk c starts at iteration off_c = the sum of those before it
 *   slot_iters              iterations per pair the slot outputs hold: super_len <= slot_iters <= the pass's capacity (sched::chunk_capacity of the options)
 * with K = the sample size (3, 5, 6, 7), MPS = the model slots per sample (4, 12, 16, 4), G = ceil(n_max / 16), S = slot_iters * MPS:
 *   pts [batch][n_max][6], dep [batch][n_max][2] (monodepth kinds; NULL otherwise), rfrag [batch][G][64][4] u32, states [batch]: behind the prep
 *   table_of_pair [batch], table_n [batch] (the first *n_tables entries)
 *   samples [batch][super_len][K]    table t's chunk c at [t][off_c]: the chunks of a table side by side (rows from *n_tables on are not written)
 *   slot_inl [n_chunks][batch][S]    the slot states behind each chunk's solver;  models [batch][S]: behind the last
 *   tags [n_chunks][batch][S]        the chunk's tag list: pair p's first model_count[c][p][0] entries are its live slots, in no defined order
 *   model_count [n_chunks][batch][2]
 * MDRP_ERR_INVALID before any device work: what mdrp_estimate_batch refuses; batch or n_max < 1; a NULL output; no chunk, more than 8, a length < 1;
 * slot_iters outside its range; for MDRP_RELPOSE_5PT with several chunks, a first chunk longer than the pass's first-chunk Reduce5 region.
 * tests/test_gpu_front_stages.py pins every stage to tests/front_stages_ref.py. */
#define MDRP_FRONT_FILL 0xA5
typedef struct { /* what k_prep / kc_prep leave of a pair (field for field the kernels' pair state) */
    int32_t n, table, active, n_triggers;
    double eps, sq_thr, scale_reproj, lo_loss_scale, final_loss_scale, norm;
    double box[4], cen[4];
    uint64_t best_min_cnt;
    double best_min_score;
    uint64_t dyn_max_iter, iterations, refinements, num_inliers;
    double inlier_ratio, model_score;
    mdrp_model best;
} mdrp_front_state;
typedef struct {
    /* in */
    int32_t kind, batch, n_max, n_chunks;
    int32_t slot_iters, pad_;
    const double *x1, *x2, *d1, *d2;
    const int32_t *n_per_pair;       /* [batch] or NULL */
    const mdrp_camera *cam1, *cam2;
    const int32_t *chunk_lens;
    /* out */
    double *pts, *dep;
    uint32_t *rfrag;
    mdrp_front_state *states;
    int32_t *table_of_pair, *table_n, *n_tables;
    uint32_t *samples;
    int32_t *slot_inl;
    mdrp_model *models;
    uint32_t *tags;
    int32_t *model_count;
} mdrp_front_run;
int mdrp_front_stages(mdrp_handle *h, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, mdrp_front_run *io);

/* Hybrid LM refinement of `count` models, each over the correspondences of ONE pair (refine_monodepth_*relpose
 * @0x261030/@0x2592e0/@0x260fa0).  Host memory.  models in/out.  For MDRP_RELPOSE_5PT / MDRP_FUNDAMENTAL_7PT: the Sampson-only
 * refine_relpose @0x258f50 / refine_fundamental @0x2590d0 (d1, d2, scale_reproj, weight_sampson, estimate_shift ignored). */
int mdrp_refine_models(mdrp_handle *h, int kind, mdrp_model *models, int count, const double *x1, const double *x2,
                       const double *d1, const double *d2, int n, double scale_reproj, double weight_sampson,
                       const mdrp_bundle_opt *opt, int estimate_shift, double *final_cost /*[count] or NULL*/);

/* Timing of the last mdrp_estimate_batch* call on this handle, measured with HIP events on the handle's stream:
 * total milliseconds in the scoring-sweep kernel, number of its launches, and (model x correspondence) evaluations. */
int mdrp_last_sweep_stats(mdrp_handle *h, double *sweep_ms, int64_t *launches, int64_t *evaluations);

/* The same with the two scoring kernels apart (HIP events on the handle's stream around every launch of each kernel):
 * k_count — candidate counts of all hypotheses on the matrix cores (v_mfma_f32_16x16x32_bf16) — and k_score — the exact
 * fp64 sweep of the hypotheses k_count could not retire. */
typedef struct {
    double count_ms;           /* total time in k_count */
    int64_t count_launches;
    double sweep_ms;           /* total time in k_score */
    int64_t sweep_launches;
    int64_t evals_algorithmic; /* (model x correspondence) evaluations the CPU loop does: sum over pairs of models * n */
    int64_t evals_mfma;        /* evaluations executed by k_count (16 x 16 tiles, padding included) */
    int64_t evals_fp64;        /* evaluations handed to k_score (survivors * n) */
    int64_t evals_bound;       /* evaluations executed by k_bound in fp32 (k_count's survivors * n) */
    /* LM refinements (refine_monodepth_*relpose @0x261030 / @0x2592e0 / @0x260fa0): HIP events around every launch of the LO
     * kernel (on the stream it runs on) and of the final-refinement kernel, and the correspondences their sweeps evaluated */
    double lo_ms;              /* total time in k_lo (or the LM engine's LO phases) */
    int64_t lo_launches;
    double final_ms;           /* total time in k_final (or the LM engine's final phase) */
    int64_t final_launches;
    double bound_ms;           /* total time in k_bound */
    int64_t bound_launches;
    double solve_ms;           /* total time in the minimal-solver kernel */
    int64_t solve_launches;
    int64_t lm_cost_evals;     /* LO kernel: correspondences evaluated by its cost sweeps (residuals only) */
    int64_t lm_accum_evals;    /* LO kernel: correspondences evaluated by its normal-equation sweeps (residuals + Jacobians + J'J) */
    int64_t final_cost_evals;  /* the same two counters of the final-refinement kernel */
    int64_t final_accum_evals;
    /* ---- appended in ABI 0.3 (mdrp_last_stats_sized only) ----
     * Fused tail (the last LO launch and the final refinements overlap on two streams): bounded waits that expired in the
     * last call.  Non-zero means kernels of the handle's streams did not run side by side (serialising profiler / debugger,
     * AMD_SERIALIZE_KERNEL, a busy shared GPU): results are unaffected, the call was slower, final_ms includes the waits, and the
     * handle runs unfused for a number of calls, then tries again: 64 after the first call with an expired wait, doubling with every further such
     * call up to 16384, back to 64 after a clean call (mdrp_capi.hip finish_timing). */
    int64_t fuse_gate_timeouts;
    int64_t fuse_wait_timeouts;
    /* ---- appended in ABI 0.5 (mdrp_last_stats_sized only) ----
     * Iterations of the first chunk of the last call — the part of a run that is scored exactly in full because nothing has set a bar yet.  The
     * monodepth estimators size it from the inlier ratios of the results of the handle's PREVIOUS call with the same estimator (a pair whose first
     * chunk holds no outlier-free sample has no bar for the rest of its run: 256 iterations where half of the correspondences are inliers, 1024
     * where one in seven is, 128 where all are), 256 without one; MDRP_CHUNKS overrides.  Results do not depend on it. */
    int64_t first_chunk;
} mdrp_stats;
/* writes min(out_size, sizeof(mdrp_stats)) bytes: pass sizeof(mdrp_stats) of the header the caller was compiled against */
int mdrp_last_stats_sized(mdrp_handle *h, mdrp_stats *out, size_t out_size);
/* the ABI 0.2 entry point: writes the ABI 0.2 struct (everything before fuse_gate_timeouts), never more.
 * With the fused tail, lo_ms and final_ms are overlapping intervals on two streams and final_ms includes the final refinements' wait
 * for their pairs: read them as one phase (lo_ms + final_ms is an upper bound of it), not as two kernel durations. */
int mdrp_last_stats(mdrp_handle *h, mdrp_stats *out);

/* ---- ABI 0.6: the device front end — estimate straight from a matcher's output and two depth maps ----
 * What every caller of the reference does on the host before the estimator (make_pair.py:96-106, make_video.py:265-275): gather the matched
 * keypoints, read each keypoint's depth at the truncated pixel, drop the correspondences whose depths are both infinite.  Here the same
 * happens on the device, so extractor, matcher and depth network outputs never leave it.  For pair b and match row m = (i, j), in row order:
 *   1. the row is padding and dropped when i < 0 or j < 0 (LightGlue's -1; no counts go in), dropped as well when i >= k1 or j >= k2;
 *   2. p1 = kp1[b][i], p2 = kp2[b][j]; the row is dropped unless x > -1 && x < w && y > -1 && y < h in its image (tested on the floating
 *      value: -0.5 is pixel 0, w - 0.001 is pixel w - 1; -1, w, NaN and +-inf are dropped); the pixel is the coordinate truncated toward zero;
 *   3. d1 = depth1[b][yi1][xi1], d2 = depth2[b][yi2][xi2], widened to double;
 *   4. filter MDRP_FILTER_BOTH_INF drops the row iff both depths are infinite (the scripts' rule: a NaN or a one-sided infinity is kept);
 *      MDRP_FILTER_FINITE keeps it only when both depths are finite;
 *   5. kept rows go, IN MATCH ORDER, to slots s = 0, 1, ...: x1[b][s] = (double)p1 - center1[b] (centres optional, subtracted in double: the
 *      focal estimators take principal-point-centred pixels), x2 likewise, d1[b][s], d2[b][s]; slot[b][m] = s, -1 for a dropped row; n[b]
 *      is the number of kept rows; slots >= n[b] are filled with x = 0, d = 1.
 * Every pointer of the descriptor is DEVICE memory. */
enum { MDRP_F32 = 0, MDRP_F64 = 1 };                        /* kp_type, depth_type */
enum { MDRP_FILTER_BOTH_INF = 0, MDRP_FILTER_FINITE = 1 };  /* filter */
typedef struct {
    const void *kp1, *kp2;         /* [B][k1][2], [B][k2][2] keypoints (x, y) in pixels of their depth map */
    int32_t kp_type;               /* MDRP_F32 | MDRP_F64 */
    int32_t k1, k2;                /* keypoints per image */
    const int32_t *matches;        /* [B][m_max][2] index pairs (i into kp1, j into kp2); a negative index marks a padding row */
    int32_t m_max;                 /* match rows per pair */
    const void *depth1, *depth2;   /* [B][h1][w1], [B][h2][w2] depth maps */
    int32_t depth_type;            /* MDRP_F32 | MDRP_F64 */
    int32_t h1, w1, h2, w2;
    const double *center1, *center2; /* [B][2] or NULL */
    int32_t filter;                /* MDRP_FILTER_BOTH_INF | MDRP_FILTER_FINITE */
} mdrp_matches;

/* The front end alone.  x1, x2: [B][m_max][2], d1, d2: [B][m_max], slot: [B][m_max] — DEVICE memory of the caller; n_host: [B] kept rows per
 * pair, HOST memory.  Queued on the handle's stream; returns after the counts have arrived (one stream synchronisation).
 * MDRP_ERR_INVALID: a NULL buffer, a negative size, an unknown type or filter. */
int mdrp_gather_matches(mdrp_handle *h, const mdrp_matches *mm, int batch, double *x1, double *x2, double *d1, double *d2, int32_t *slot,
                        int32_t *n_host);

/* Front end + estimator.  Gathers into buffers of the handle, copies the B counts to pinned host memory and synchronises the stream ONCE (the
 * host scheduler sizes its sample tables and passes from the counts; the estimator itself synchronises once per super-chunk anyway), then
 * runs exactly what mdrp_estimate_batch_async runs on (x1, x2, d1, d2, n_max = m_max, n_per_pair = the counts): same records, same option
 * refusals.  Results are read with mdrp_fetch_results / mdrp_copy_results_device.  kind: MDRP_CALIB, MDRP_SHARED_FOCAL or MDRP_VARYING_FOCAL
 * (the estimators that take depths; any other kind is MDRP_ERR_INVALID).  match_mask_dev: [B][m_max] bytes in DEVICE memory or NULL — 1 where
 * the row was kept and is an inlier of the result; n_used_host: [B] in HOST memory or NULL — the counts. */
int mdrp_estimate_matches_async(mdrp_handle *h, int kind, const mdrp_matches *mm, int batch, const mdrp_camera *cam1_host,
                                const mdrp_camera *cam2_host, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                                uint8_t *match_mask_dev, int32_t *n_used_host);

/* ---- Iteration budgets: the result at every budget of a list in ONE run (added within ABI 0.6: new symbols only).
 * budgets: n_budgets integers in HOST memory, each >= 1, strictly increasing, at most MDRP_MAX_BUDGETS of them, and ropt->max_iterations must
 * equal the last one.  Record and mask c are bit for bit what a separate call with max_iterations = budgets[c] and every other option unchanged
 * returns: the sample sequence depends on (seed, N) alone and a run's bookkeeping on earlier iterations alone, so the run with budget K is a
 * prefix of every longer run.  A pair that the dynamic stopping rule ended before a budget reports its stopped state there.
 * MDRP_ERR_INVALID, before any device work: an empty list, a zero budget, a list that does not increase, more than MDRP_MAX_BUDGETS, a last
 * budget other than ropt->max_iterations.  Every other argument, error and option refusal is mdrp_estimate_batch's.
 * out: [n_budgets][batch] records; inlier_mask: [n_budgets][batch][n_max] bytes or NULL (host or device memory as mem_space says). */
#define MDRP_MAX_BUDGETS 16
int mdrp_estimate_batch_budgets(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, const double *d1,
                                const double *d2, int batch, int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1,
                                const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, const uint64_t *budgets,
                                int n_budgets, mdrp_result *out, uint8_t *inlier_mask);
/* Device-resident variant (as mdrp_estimate_batch_async): inlier_mask_dev is [n_budgets][batch][n_max] bytes in DEVICE memory or NULL.  The
 * records stay on the device until mdrp_fetch_budget_results / mdrp_copy_budget_results_device ([n_budgets][batch] records; n_budgets and
 * batch are the call's); mdrp_fetch_results / mdrp_copy_results_device return the last budget's. */
int mdrp_estimate_batch_budgets_async(mdrp_handle *h, int kind, const double *x1_dev, const double *x2_dev, const double *d1_dev,
                                      const double *d2_dev, int batch, int n_max, const int32_t *n_per_pair_host, const mdrp_camera *cam1_host,
                                      const mdrp_camera *cam2_host, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                                      const uint64_t *budgets, int n_budgets, uint8_t *inlier_mask_dev);
int mdrp_fetch_budget_results(mdrp_handle *h, mdrp_result *out_host, int n_budgets, int batch);
int mdrp_copy_budget_results_device(mdrp_handle *h, void *dst_dev, int n_budgets, int batch);

/* ---- The device front end on per-image tables (added within ABI 0.6: new symbols only).
 * A batch of pairs as its producer holds it: a video matches every frame against one anchor, an SfM front end matches each image against
 * many others — an image's keypoints and its depth map exist ONCE, and pair b is two indices (a, c) = pairs[b] into the image set.
 * mdrp_matches wants every image's tables copied once per pair the image takes part in; this descriptor does not.
 * For pair b: if a or c is outside [0, n_images), every row of the pair is dropped — n[b] = 0, every slot is -1, the buffers hold the
 * filler (x = 0, d = 1) — and nothing is read through the bad index.  Otherwise rules 1-5 of mdrp_matches apply unchanged with
 *   kp1 = kp[a], k1 = kp_count[a], depth1 = depth[a], (h1, w1) = size[a], center1 = center[a]
 * and the same from c for image 2.  a == c and repeated pairs are legal.  Every pointer of the descriptor is DEVICE memory. */
typedef struct {
    const void *kp;                /* [I][k_max][2] keypoints (x, y) in pixels of their image's depth map */
    int32_t kp_type;               /* MDRP_F32 | MDRP_F64 */
    int32_t k_max;                 /* keypoint rows allocated per image */
    const int32_t *kp_count;       /* [I] valid keypoints of each image, clamped to [0, k_max]; NULL = k_max for all */
    const void *depth;             /* [I][h_max][w_max] depth maps: the row stride is always w_max */
    int32_t depth_type;            /* MDRP_F32 | MDRP_F64 */
    int32_t h_max, w_max;          /* rows and columns allocated per map */
    const int32_t *size;           /* [I][2] (h, w): valid region of each map, clamped to [0, h_max] x [0, w_max]; NULL = the full map */
    const double *center;          /* [I][2] or NULL */
    int32_t n_images;              /* I */
    const int32_t *pairs;          /* [B][2] image indices (a, c) */
    const int32_t *matches;        /* [B][m_max][2] index pairs (i into kp[a], j into kp[c]); a negative index marks a padding row */
    int32_t m_max;                 /* match rows per pair */
    int32_t filter;                /* MDRP_FILTER_BOTH_INF | MDRP_FILTER_FINITE */
} mdrp_image_pairs;

/* Shaped exactly like mdrp_gather_matches and mdrp_estimate_matches_async: same outputs, same one stream synchronisation (the counts), then
 * the resident estimator on the gathered buffers with n_max = m_max and the counts.  Cameras stay ONE RECORD PER PAIR ([B], host memory): a
 * caller with per-image cameras expands them by pairs.  MDRP_ERR_INVALID, before any device work: a NULL descriptor, an unknown type or
 * filter, a negative size or n_images, batch > 0 and m_max > 0 with pairs or matches NULL, kp NULL with n_images > 0 and k_max > 0, depth NULL
 * with n_images > 0, h_max > 0 and w_max > 0; a kind other than MDRP_CALIB, MDRP_SHARED_FOCAL, MDRP_VARYING_FOCAL. */
int mdrp_gather_image_pairs(mdrp_handle *h, const mdrp_image_pairs *ip, int batch, double *x1, double *x2, double *d1, double *d2,
                            int32_t *slot, int32_t *n_host);
int mdrp_estimate_image_pairs_async(mdrp_handle *h, int kind, const mdrp_image_pairs *ip, int batch, const mdrp_camera *cam1_host,
                                    const mdrp_camera *cam2_host, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                                    uint8_t *match_mask_dev, int32_t *n_used_host);

/* ---- Refine and verify caller-supplied models (added within ABI 0.6: new symbols only).
 * One model per pair goes in, and the call runs exactly what the estimator runs from the moment RANSAC has picked its winner: the tail of
 * ransac<> plus the wrapper's inlier-only refinement.  Nothing is sampled.  For pair b with n = n_per_pair[b] correspondences, the caller's
 * model M0 (an mdrp_model in the caller's units, as the estimators return it: focals in pixels for the two focal kinds) and `stages`:
 *   1. Prep, exactly the estimator's: unproject by the cameras (MDRP_CALIB) or divide by the normalisation scale (focal kinds; M0's focals are
 *      divided by it as well); thresholds and loss scales as the estimator computes them from max_epipolar_error, max_reproj_error,
 *      monodepth_weight_sampson (through float, clamped at 0), monodepth_estimate_shift (MDRP_CALIB only) and the caller's BundleOptions.
 *      Every other RansacOptions field is ignored — iterations, seed, stopping rule, sampler switches: nothing samples, so nothing is refused.
 *   2. S0, C0 = MSAC score and inlier count of M0 at the squared threshold: the estimator's exact fp64 sweep in record order (pose scoring
 *      with cheirality for MDRP_CALIB, F from pose and focals for the focal kinds).
 *   3. MDRP_STAGE_LO, unless M0.q[0] is NaN: M1 = LM from M0 over all n records (TRUNCATED loss at the LO's loss scale, 25 iterations, the LO's
 *      fixed tolerances: ransac<>'s LO).  M1 is adopted with its own (S1, C1) iff S1 < S0; otherwise M0 stays with (S0, C0).  (The
 *      estimator's record keeps the old score there, a reference quirk; here the adopted model's own score is reported.)
 *   4. mask = get_inliers of the model kept so far; bytes at or past n are 0.
 *   5. MDRP_STAGE_INLIERS, when the count exceeds 3 (MDRP_CALIB, MDRP_SHARED_FOCAL) or 7 (MDRP_VARYING_FOCAL): LM over the masked records with
 *      the caller's BundleOptions at the estimator's final loss scale — the wrappers' inlier-only refinement.
 *   6. Record: model = the final model, focals multiplied by the normalisation scale; model_score, num_inliers, inlier_ratio = count / n and
 *      the mask describe the model that ENTERED stage 5 (the estimator's convention; call again with stages = 0 for the numbers of the returned
 *      model); iterations = 0; refinements = LM runs executed (0 to 2).
 *   7. initial_score[b] = S0, initial_inliers[b] = C0 (both optional).  A pair no LM ran on — stages = 0 (verification only), a NaN start
 *      model — returns the caller's model BIT FOR BIT, without a focal round trip.  n < 3: the caller's model bit for bit, zeroed stats,
 *      model_score = S0 = DBL_MAX, a zero mask (the estimators' rule).  A NaN start model scores n * threshold^2 with 0 inliers.
 * The default stages = MDRP_STAGE_LO | MDRP_STAGE_INLIERS is the estimator's tail; MDRP_STAGE_INLIERS alone, started from ransac<>'s winner,
 * gives the estimator's result.
 * kind: MDRP_CALIB, MDRP_SHARED_FOCAL or MDRP_VARYING_FOCAL (any other kind is MDRP_ERR_INVALID).  MDRP_ERR_INVALID, before any device work:
 * a NULL required buffer, a negative size, n_per_pair out of range, stages outside 0..3.
 * x1, x2, d1, d2, models ([B]) and inlier_mask ([B][n_max] bytes or NULL) live in mem_space; n_per_pair, cameras, out ([B]), initial_score
 * and initial_inliers ([B] each, or NULL) in HOST memory.  The call runs on the handle's stream, replaces the handle's last results and is
 * synchronous with respect to `out`. */
enum { MDRP_STAGE_LO = 1, MDRP_STAGE_INLIERS = 2 };
int mdrp_refine_batch(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, const double *d1, const double *d2,
                      int batch, int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2,
                      const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, const mdrp_model *models, int stages, mdrp_result *out,
                      uint8_t *inlier_mask, double *initial_score, int32_t *initial_inliers);
/* Device-resident variant: nothing is copied back and the call does not wait.  The records stay in the handle's device buffers until
 * mdrp_fetch_results / mdrp_copy_results_device; initial_score_dev / initial_inliers_dev are [B] in DEVICE memory or NULL. */
int mdrp_refine_batch_async(mdrp_handle *h, int kind, const double *x1_dev, const double *x2_dev, const double *d1_dev, const double *d2_dev,
                            int batch, int n_max, const int32_t *n_per_pair_host, const mdrp_camera *cam1_host, const mdrp_camera *cam2_host,
                            const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, const mdrp_model *models_dev, int stages,
                            uint8_t *inlier_mask_dev, double *initial_score_dev, int32_t *initial_inliers_dev);

/* ---- Estimate with a prior (added within ABI 0.6: new symbols only).
 * mdrp_estimate_batch with one model per pair that the search starts from: the LO-RANSAC run unchanged, with the caller's model scored and
 * LO-refined first, exactly as ransac<> treats an initial model under score_initial_model — and NOT reset to the identity, as the reference's
 * wrappers reset it.  A good prior retires garbage hypotheses from the first chunk on and lowers the dynamic iteration bound at once; a bad
 * prior costs one LM and changes nothing else; a wrong prior cannot give a wrong answer, because everything is still sampled
 * (mdrp_refine_batch is the call that trusts the model).  For pair b with n = n_per_pair[b] correspondences and prior P (an mdrp_model in the
 * caller's units, as the estimators return it: focals in pixels for the two focal kinds):
 *   - n < 3: the estimators' record (identity model, zero stats, model_score = DBL_MAX).  P is not read.
 *   - P.q[0] is NaN: the pair has no prior and behaves as in mdrp_estimate_batch, ropt->score_initial_model included.
 *   - otherwise the pair ignores ropt->score_initial_model, and its state before iteration 0 is:
 *       1. focal kinds: P.f1, P.f2 divided by the pair's normalisation scale.
 *       2. (S0, C0) = exact MSAC score and inlier count of P at the squared threshold, in record order.
 *       3. more = C0 > 0, better = S0 < DBL_MAX.  Neither (a NaN score): nothing changes, no LM.  Otherwise the records of the minimal
 *          models become best_minimal_inlier_count = C0 (if more) and best_minimal_msac_score = S0 (if better), and P is the best model
 *          with model_score = S0 and num_inliers = C0.
 *       4. LO: the 25-iteration TRUNCATED LM at the LO's loss scale from P over all records gives M1 with (S1, C1); refinements = 1.  M1 is
 *          adopted with its score and count iff S1 < model_score.  The LO never touches the records of the minimal models.
 *       5. inlier_ratio = num_inliers / n, and the dynamic iteration bound follows from it by ransac<>'s rule.
 *       6. This is not an iteration: iterations stays 0 and no stop test runs.  With max_iterations = 0 the loop ends here, and the closing LO,
 *          the mask and the inlier-only refinement run on this state.
 *   - everything behind that — sampling, scoring, LO triggers, stopping, closing LO, get_inliers, inlier-only refinement, focal
 *     un-normalisation, the record — is mdrp_estimate_batch's, unchanged.  The state a prior leaves does not depend on the batch.
 * kind: MDRP_CALIB, MDRP_SHARED_FOCAL or MDRP_VARYING_FOCAL.  MDRP_ERR_INVALID, before any device work: any other kind, batch > 0 with a NULL
 * prior, and everything mdrp_estimate_batch refuses; the option refusals (progressive_sampling: MDRP_ERR_UNSUPPORTED) are the estimator's own.
 * x1, x2, d1, d2, prior ([B]) and inlier_mask ([B][n_max] bytes or NULL) live in mem_space; n_per_pair, cameras and out ([B]) in HOST memory.
 * Host buffers are copied in one piece on the handle's stream before the run (no sliced front).  Iteration budgets do not combine with priors. */
int mdrp_estimate_batch_prior(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, const double *d1, const double *d2,
                              int batch, int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1, const mdrp_camera *cam2,
                              const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, const mdrp_model *prior, mdrp_result *out,
                              uint8_t *inlier_mask);
/* Device-resident variant, as mdrp_estimate_batch_async: results through mdrp_fetch_results / mdrp_copy_results_device. */
int mdrp_estimate_batch_prior_async(mdrp_handle *h, int kind, const double *x1_dev, const double *x2_dev, const double *d1_dev,
                                    const double *d2_dev, int batch, int n_max, const int32_t *n_per_pair_host, const mdrp_camera *cam1_host,
                                    const mdrp_camera *cam2_host, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt,
                                    const mdrp_model *prior_dev, uint8_t *inlier_mask_dev);

/* ---- Estimate in match-score order: PROSAC (added within ABI 0.6: new symbols only).
 * mdrp_estimate_batch on the records of every pair taken in descending score order, with the sample sequence of the reference's
 * RansacOptions::progressive_sampling (RandomSampler::initialize_prosac / generate_sample) in place of the uniform one.  For a pair with n records
 * and scores s[0..n), higher is better:
 *   - order = stable argsort of -key, key = s with NaN replaced by -inf; -0.0 and +0.0 tie; ties go by ascending caller index.  order[r] is the
 *     caller index of the record at rank r.  scores == NULL: the records are in quality order already, nothing is ranked or permuted.
 *   - the sampler (sample size K = 3), with M = ropt->max_prosac_iterations, all in fp64 and in exactly this order of operations:
 *       growth[0..max(n,K)):  T = (double)M;  for i in 0..K-1: T *= (double)(K-i) / (double)(n-i);  Tp = 1;  growth[0..K) = 1;
 *                             for i in K..n-1: Tn = T*(i+1.0)/(i+1.0-K); Tp += ceil(Tn - T); growth[i] = Tp; T = Tn
 *       state:   rng = ropt->seed, k = 1, sub = K
 *       sample:  if k < M: K-1 distinct indices from [0, sub-1) by the estimators' splitmix64 draw (redraw on a duplicate, same modulo rule), then
 *                index K-1 := sub-1;  k += 1;  if k < M and k > growth[sub-1]: sub = min(sub+1, n)
 *                else: the estimators' uniform draw of K from n
 *     M <= 1 is uniform sampling from the first sample on: the call then equals mdrp_estimate_batch on the pre-sorted records bit for bit.
 *   - everything else runs on the ordered records and is mdrp_estimate_batch's, unchanged: normalisation sums, the MSAC sums in record order, LO,
 *     stopping, closing LO, get_inliers, the inlier-only refinement, the record.  inlier_mask[order[r]] = mask of rank r: the mask is in the
 *     caller's order; bytes at or past n are 0.
 * These entry points are what progressive_sampling selects in the reference, so they sample progressively whether ropt->progressive_sampling is 0
 * or 1 (a reference caller's options pass unabridged); every other entry point but the ranked front end (below) still refuses the switch.  kind: MDRP_CALIB, MDRP_SHARED_FOCAL or
 * MDRP_VARYING_FOCAL; any other kind is MDRP_ERR_INVALID (the baselines have mdrp_estimate_classic_ranked, below), as is everything mdrp_estimate_batch refuses (NULL depths, n_per_pair out of range, ...).
 * A refusal leaves the handle usable.  x1, x2, d1, d2, scores ([B][n_max] doubles or NULL) and inlier_mask ([B][n_max] bytes or NULL) live in
 * mem_space; n_per_pair, cameras and out ([B]) in HOST memory.  Host buffers are copied in one piece on the handle's stream (no sliced front).
 * Iteration budgets and priors do not combine with scores.  The ordered copies of the correspondences are the handle's and are allocated before
 * the passes are sized from the free memory. */
int mdrp_estimate_batch_ranked(mdrp_handle *h, int kind, int mem_space, const double *x1, const double *x2, const double *d1, const double *d2,
                               const double *scores, int batch, int n_max, const int32_t *n_per_pair, const mdrp_camera *cam1,
                               const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, mdrp_result *out,
                               uint8_t *inlier_mask);
/* Device-resident variant, as mdrp_estimate_batch_async: results through mdrp_fetch_results / mdrp_copy_results_device. */
int mdrp_estimate_batch_ranked_async(mdrp_handle *h, int kind, const double *x1_dev, const double *x2_dev, const double *d1_dev,
                                     const double *d2_dev, const double *scores_dev, int batch, int n_max, const int32_t *n_per_pair_host,
                                     const mdrp_camera *cam1_host, const mdrp_camera *cam2_host, const mdrp_ransac_opt *ropt,
                                     const mdrp_bundle_opt *bopt, uint8_t *inlier_mask_dev);
/* Inspection: the device sampler alone for one table of n records, drawn chunk by chunk (chunk_lens[n_chunks], each >= 1) through the launch the
 * scheduler uses, its state carried on the device between chunks.  out: [sum of chunk_lens][3] uint32 in HOST memory; n < 3 writes nothing. */
int mdrp_prosac_samples(mdrp_handle *h, uint64_t seed, int n, uint64_t max_prosac_iterations, const int32_t *chunk_lens, int n_chunks,
                        uint32_t *out);
/* Inspection: the ranking kernel alone.  scores [B][n_max] doubles and order [B][n_max] int32 live in mem_space; order[b][r] = -1 for r >= n. */
int mdrp_rank_scores(mdrp_handle *h, int mem_space, const double *scores, int batch, int n_max, const int32_t *n_per_pair, int32_t *order);

/* ---- The 5- / 6- / 7-point baselines in match-score order (added within ABI 0.6: new symbols only) are declared and documented in
 * mdrp_classic_ranked.h, which this header includes at its end: the ranked estimate for kinds 3 - 5, blocking and device-resident, and the
 * progressive sampler alone for a sample size of 3, 5, 6 or 7. */

/* ---- The device front end with match scores: PROSAC from a matcher's confidences (added within ABI 0.6: new symbols only).
 * mdrp_gather_matches / mdrp_gather_image_pairs and the two front-end estimates, with one score per MATCH ROW, higher is better:
 * scores_dev is [B][m_max] in DEVICE memory, floats or doubles as score_type says (MDRP_F32 | MDRP_F64; float widens exactly).  For pair b:
 *   - rules 1-4 of mdrp_matches, for mdrp_image_pairs behind the image-index rule, decide which rows are kept, exactly as without scores.  A row's
 *     score plays no part in whether it is kept, and the score of a dropped row is never looked at.
 *   - key(m) = (double)scores[b][m] with NaN (either sign) replaced by -inf; -0.0 and +0.0 tie.
 *   - rank(m) = #{m' kept : key(m') > key(m), or key(m') == key(m) and m' < m}: the order of mdrp_estimate_batch_ranked on the kept rows' scores in
 *     match order (a stable descending sort).
 *   - slot[b][m] = rank(m) for a kept row, -1 for a dropped one; the record of row m (rule 5's x1, x2, d1, d2) is at index rank(m) of pair b's
 *     buffers; n[b] = kept rows; slots >= n[b] hold the filler (x = 0, d = 1).
 * The estimates then run exactly what mdrp_estimate_batch_ranked_async runs with scores == NULL (records in quality order already) on those buffers
 * with n_max = m_max and n_per_pair = the counts: the progressive sampler, whether ropt->progressive_sampling is 0 or 1; max_prosac_iterations <= 1
 * is the uniform sampler on the ordered records.  That is, bit for bit, mdrp_estimate_batch_ranked on the unranked gather with the kept rows' scores.
 * match_mask_dev[b][m] = 1 iff row m was kept and its correspondence is an inlier; n_used_host: the counts.  Each kept row is written once, at its
 * rank: no order buffer, no ordered copy, no scatter of the mask.  The handle holds one 8-byte key per match row for the call.
 * scores_dev == NULL: the match rows are in quality order already — the unranked gather (score_type is not read), followed in the estimates by the
 * progressive sampler.
 * MDRP_ERR_INVALID, before any device work: everything mdrp_gather_matches / mdrp_gather_image_pairs / the front-end estimates refuse (descriptor,
 * kind), a score_type other than MDRP_F32 / MDRP_F64 with scores_dev != NULL, and the estimator's own refusals taken with progressive_sampling
 * cleared (cameras for MDRP_CALIB; MDRP_ERR_UNSUPPORTED for an option that is not built).  A refusal leaves the handle usable; an error behind the
 * first device work returns after the handle's streams have drained.  Same stream behaviour as the unranked forms: one synchronisation (the
 * counts).  Iteration budgets and priors do not combine with scores. */
int mdrp_gather_matches_ranked(mdrp_handle *h, const mdrp_matches *mm, const void *scores_dev, int score_type, int batch, double *x1, double *x2,
                               double *d1, double *d2, int32_t *slot, int32_t *n_host);
int mdrp_estimate_matches_ranked_async(mdrp_handle *h, int kind, const mdrp_matches *mm, const void *scores_dev, int score_type, int batch,
                                       const mdrp_camera *cam1_host, const mdrp_camera *cam2_host, const mdrp_ransac_opt *ropt,
                                       const mdrp_bundle_opt *bopt, uint8_t *match_mask_dev, int32_t *n_used_host);
int mdrp_gather_image_pairs_ranked(mdrp_handle *h, const mdrp_image_pairs *ip, const void *scores_dev, int score_type, int batch, double *x1,
                                   double *x2, double *d1, double *d2, int32_t *slot, int32_t *n_host);
int mdrp_estimate_image_pairs_ranked_async(mdrp_handle *h, int kind, const mdrp_image_pairs *ip, const void *scores_dev, int score_type, int batch,
                                           const mdrp_camera *cam1_host, const mdrp_camera *cam2_host, const mdrp_ransac_opt *ropt,
                                           const mdrp_bundle_opt *bopt, uint8_t *match_mask_dev, int32_t *n_used_host);

#ifdef __cplusplus
}
#endif
#include "mdrp_classic_ranked.h"
#include "mdrp_classic_models.h"
#include "mdrp_classic_frontend.h" /* the device front end of the 5- / 6- / 7-point baselines: matcher output without depth maps */
#include "mdrp_classic_focals.h"   /* the varying-focal baseline: focals and pose from the 7-point estimator's fundamental matrix */
#include "mdrp_dense.h"            /* the front end for dense matchers: a warp sampled by certainty on the device */
#endif
