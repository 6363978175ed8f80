// mdrp_capi_entry.h — the entry layer of the C ABI: everything between the extern "C" estimator, refine, gather and rank symbols of include/mdrp*.h
// (mdrp_capi.hip, right behind this file) and estimate_device / the refine kernels ("the entry layer").  Included ONCE, by mdrp_capi.hip,
// behind the handle, the scheduler and MDRP_ENTER: it is a part of that translation unit, not a header to include elsewhere.
//
// An entry point is: refuse (one routine, a descriptor per family) | fill the call record by name | [blocking, host buffers: stage] | run | [blocking: finish].
// A failing call leaves through MDRP_ENTER's DrainOnFailure whichever return it takes: no call site drains by hand.

// ---- results of the last call
static int fetch_results_locked(mdrp_handle *h, mdrp_result *out, int batch) {
    if (!out || batch < 0 || batch > h->last_batch) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    HIPCHK(hipMemcpyAsync(out, h->results.p, sizeof(ResultDev) * batch, hipMemcpyDeviceToHost, h->stream));
    return finish_timing(h);
}

// iteration budgets
static_assert(MDRP_MAX_BUDGETS == MAX_BUDGETS, "budget limit of the header and of the kernels");

static int budget_results_locked(mdrp_handle *h, void *dst, int n_budgets, int batch, hipMemcpyKind where) {
    if (!dst || batch < 0 || n_budgets < 1 || n_budgets != h->last_budgets || batch != h->last_batch) {
        g_err = "budget results: n_budgets and batch must be those of the handle's last budgets call";
        return MDRP_ERR_INVALID;
    }
    if (batch > 0) HIPCHK(hipMemcpyAsync(dst, h->bresults.p, sizeof(ResultDev) * n_budgets * batch, where, h->stream));
    return finish_timing(h);
}

// ---- the call record of an entry point
// the arguments every estimator and refine entry point takes, in the ABI's own order; what else a call uses, its entry point names
static EstimateCall call_of(int kind, const double *x1, const double *x2, const double *d1, const double *d2, int batch, int n_max, const int32_t *n_per_pair,
                            const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt) {
    EstimateCall c;
    c.kind = kind; c.x1 = x1; c.x2 = x2; c.d1 = d1; c.d2 = d2; c.batch = batch; c.n_max = n_max; c.n_per_pair = n_per_pair;
    c.cam1 = cam1; c.cam2 = cam2; c.ro = ropt; c.bo = bopt;
    return c;
}

// A ranked run: progressive_sampling is what a ranked entry point builds, it is not handed on to the estimator (which refuses it); the sampler takes
// the caller's max_prosac_iterations.  The one place that clears the switch: the refusals (refusals_as_run) and the runs both go through here.
struct RankedRun {
    mdrp_ransac_opt plain;
    uint64_t max_prosac;
    explicit RankedRun(const mdrp_ransac_opt &ro) : plain(ro), max_prosac(ro.max_prosac_iterations) { plain.progressive_sampling = 0; }
    void apply(EstimateCall &c) const { c.ro = &plain; c.prosac = &max_prosac; }
};

// the estimator's own refusals, before any device work, on the options as the estimator will see them
static int refusals_as_run(mdrp_handle *h, EstimateCall c, bool ranked) {
    if (!ranked || !c.ro) return estimate_refusals(h, c);
    const RankedRun rr(*c.ro);
    c.ro = &rr.plain;
    return estimate_refusals(h, c);
}

// ---- what the entry points refuse before any device work
static_assert(MDRP_STAGE_LO == STAGE_LO && MDRP_STAGE_INLIERS == STAGE_INLIERS, "stage flags of the header and of the kernel");

static int check_stages(int stages) {
    if (stages < 0 || stages > (MDRP_STAGE_LO | MDRP_STAGE_INLIERS)) { g_err = "refine: stages must be a combination of MDRP_STAGE_LO and MDRP_STAGE_INLIERS"; return MDRP_ERR_INVALID; }
    return MDRP_OK;
}

// The checks the families share.  A family's descriptor lists the ones it makes IN ITS ORDER: the families grew with different orders (the refine calls
// look at the stages before the models, the baselines' behind n_per_pair; the priors look at n_per_pair before the cameras, the refine calls behind them)
// and which of two refusals wins is part of the ABI (tests/test_gpu_refusals.py pins every pair).
enum Check : unsigned char {
    CK_END, CK_HANDLE, CK_OPTIONS, CK_KIND, CK_SIZES, CK_N_PER_PAIR, CK_MODELS,
    CK_POINTS,          // null correspondences (and depths, for the monodepth estimators)
    CK_POINTS_BLOCKING, // ... in the blocking form only: the device-resident form takes them on trust
    CK_CAMERAS, CK_STAGES, CK_PRIOR_SPACE,
    CK_ESTIMATOR,       // estimate_refusals (ranked families: with progressive_sampling cleared)
    CK_MEM_OUT          // the blocking form's mem_space and out
};
struct Refusals {
    int first_kind; // MDRP_CALIB: the family takes the monodepth estimators, MDRP_RELPOSE_5PT: the baselines
    bool ranked;
    const char *kind, *sizes, *models, *points; // the family's wording
    Check order[12];
};
// what an entry point takes beside the call record
struct EntryArgs {
    const void *models = nullptr; // the caller's models or priors
    int stages = 0;
    bool blocking = false;
    int mem_space = MDRP_MEM_DEVICE;
    const void *out = nullptr;
};
static EntryArgs resident_args(const void *models = nullptr, int stages = 0) {
    EntryArgs a;
    a.models = models; a.stages = stages;
    return a;
}
static EntryArgs blocking_args(int mem_space, const void *out, const void *models = nullptr, int stages = 0) {
    EntryArgs a = resident_args(models, stages);
    a.blocking = true; a.mem_space = mem_space; a.out = out;
    return a;
}

static int refuse(const Refusals &r, mdrp_handle *h, const EstimateCall &c, const EntryArgs &a) {
    const bool mono = r.first_kind == MDRP_CALIB;
    const char *why = nullptr;
    for (int i = 0; !why && r.order[i] != CK_END; ++i) {
        switch (r.order[i]) {
        case CK_HANDLE: if (!h) why = "invalid argument"; break;
        case CK_OPTIONS: if (!c.ro || !c.bo) why = "invalid argument"; break;
        case CK_KIND: if (c.kind < r.first_kind || c.kind > r.first_kind + 2) why = r.kind; break;
        case CK_SIZES: if (c.batch < 0 || c.n_max < 0) why = r.sizes; break;
        case CK_N_PER_PAIR: why = n_per_pair_out_of_range(c.n_per_pair, c.batch, c.n_max); break;
        case CK_MODELS: if (c.batch > 0 && !a.models) why = r.models; break;
        case CK_POINTS_BLOCKING: if (!a.blocking) break; // fall through
        case CK_POINTS: if (c.batch > 0 && c.n_max > 0 && (!c.x1 || !c.x2 || (mono && (!c.d1 || !c.d2)))) why = r.points; break;
        case CK_CAMERAS: why = missing_cameras(c.kind, c.batch, c.cam1, c.cam2); break;
        case CK_STAGES: if (int rc = check_stages(a.stages)) return rc; break;
        case CK_PRIOR_SPACE: if (c.prior_space != 0 && c.prior_space != 1) why = "classic_prior: prior_space must be 0 (the caller's units) or 1 (the estimator's normalised coordinates)"; break;
        case CK_ESTIMATOR: if (int rc = refusals_as_run(h, c, r.ranked)) return rc; break;
        case CK_MEM_OUT: if (a.blocking && (!a.out || (a.mem_space != MDRP_MEM_HOST && a.mem_space != MDRP_MEM_DEVICE))) why = "invalid argument"; break;
        case CK_END: break;
        }
    }
    if (why) { g_err = why; return MDRP_ERR_INVALID; }
    return MDRP_OK;
}

#define MDRP_MONO_KINDS "(MDRP_CALIB, MDRP_SHARED_FOCAL, MDRP_VARYING_FOCAL)"
#define MDRP_CLASSIC_KINDS "(MDRP_RELPOSE_5PT, MDRP_SHARED_6PT, MDRP_FUNDAMENTAL_7PT)"
static const char MONO_POINTS[] = "monodepth estimator needs correspondences and depths";
// estimate with a prior (mdrp_prior.h): the option refusals are the estimator's own
static const Refusals REFUSE_PRIOR{MDRP_CALIB, false, "prior: only the monodepth estimators " MDRP_MONO_KINDS, "prior: a negative size", "prior: prior is NULL", MONO_POINTS,
                                   {CK_HANDLE, CK_KIND, CK_SIZES, CK_MODELS, CK_N_PER_PAIR, CK_ESTIMATOR, CK_MEM_OUT, CK_POINTS_BLOCKING}};
// refine and verify caller-supplied models (mdrp_from_model.h): no samples are drawn, the sampling options are not looked at
static const Refusals REFUSE_REFINE{MDRP_CALIB, false, "refine: only the monodepth estimators' models " MDRP_MONO_KINDS, "refine: a negative size", "refine: models is NULL",
                                    "refine: correspondences and depths are required",
                                    {CK_HANDLE, CK_OPTIONS, CK_KIND, CK_SIZES, CK_STAGES, CK_MODELS, CK_POINTS, CK_CAMERAS, CK_N_PER_PAIR, CK_MEM_OUT}};
// estimate in match-score order (mdrp_prosac.h), the monodepth estimators and the baselines
static const Refusals REFUSE_RANKED{MDRP_CALIB, true,
                                    "ranked: only the monodepth estimators " MDRP_MONO_KINDS "; the 5- / 6- / 7-point baselines have no depths: mdrp_estimate_classic_ranked takes them",
                                    "ranked: a negative size", nullptr, MONO_POINTS,
                                    {CK_HANDLE, CK_OPTIONS, CK_KIND, CK_SIZES, CK_N_PER_PAIR, CK_ESTIMATOR, CK_MEM_OUT, CK_POINTS_BLOCKING}};
static const Refusals REFUSE_CLASSIC_RANKED{MDRP_RELPOSE_5PT, true, "classic_ranked: only the baselines " MDRP_CLASSIC_KINDS "; mdrp_estimate_batch_ranked takes the monodepth estimators",
                                            "classic_ranked: a negative size", nullptr, "classic_ranked: correspondences are NULL",
                                            {CK_HANDLE, CK_OPTIONS, CK_KIND, CK_SIZES, CK_N_PER_PAIR, CK_ESTIMATOR, CK_MEM_OUT, CK_POINTS_BLOCKING}};
// the baselines from a caller's model (include/mdrp_classic_models.h; mdrp_classic_models.h)
#define MDRP_CLASSIC_MODELS_WORDING                                                                                                                           \
    "classic models: only the baselines " MDRP_CLASSIC_KINDS "; mdrp_refine_batch and mdrp_estimate_batch_prior take the monodepth estimators",                \
        "classic models: a negative size", "classic models: models / prior is NULL", "classic models: correspondences are NULL"
static const Refusals REFUSE_REFINE_CLASSIC{MDRP_RELPOSE_5PT, false, MDRP_CLASSIC_MODELS_WORDING,
                                            {CK_HANDLE, CK_OPTIONS, CK_KIND, CK_SIZES, CK_MODELS, CK_POINTS, CK_CAMERAS, CK_N_PER_PAIR, CK_STAGES, CK_MEM_OUT}};
static const Refusals REFUSE_CLASSIC_PRIOR{MDRP_RELPOSE_5PT, false, MDRP_CLASSIC_MODELS_WORDING,
                                           {CK_HANDLE, CK_OPTIONS, CK_KIND, CK_SIZES, CK_MODELS, CK_POINTS, CK_CAMERAS, CK_N_PER_PAIR, CK_PRIOR_SPACE, CK_ESTIMATOR, CK_MEM_OUT}};
#undef MDRP_CLASSIC_MODELS_WORDING
#undef MDRP_MONO_KINDS
#undef MDRP_CLASSIC_KINDS

// ---- blocking calls: host buffers in, masks and records out
// A blocking call on host buffers, other than the sliced front of mdrp_estimate_batch[_budgets]: the inputs are copied in plainly, in one piece, on the
// handle's stream into the handle's staging buffers, and the call - repointed - then runs the device-resident path.  (The sliced front prepares and solves
// slices on other streams, which a kernel between k_prep and the first solver - a prior, a ranking - cannot follow.)  d1 / d2 null: a baseline call, no depths;
// `models` ([batch], into fm_models) and `scores` ([batch][n_max], into pr_scores) where the call has them.
static int stage_host_call(mdrp_handle *h, EstimateCall &c, const Model **models, const double **scores) {
    if (c.batch <= 0) return MDRP_OK;
    const size_t np = (size_t)c.batch * c.n_max, b = (size_t)c.batch;
    const bool with_scores = scores && *scores && np > 0;
    hipStream_t s = h->stream;
    int rc;
    if ((rc = h->in_x1.ensure(sizeof(double) * 2 * np + 16)) || (rc = h->in_x2.ensure(sizeof(double) * 2 * np + 16)) ||
        (c.d1 && ((rc = h->in_d1.ensure(sizeof(double) * np + 16)) || (rc = h->in_d2.ensure(sizeof(double) * np + 16)))) ||
        (models && (rc = h->fm_models.ensure(sizeof(Model) * b))) || (with_scores && (rc = h->pr_scores.ensure(sizeof(double) * np))))
        return rc;
    if (np > 0) {
        HIPCHK(hipMemcpyAsync(h->in_x1.p, c.x1, sizeof(double) * 2 * np, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(h->in_x2.p, c.x2, sizeof(double) * 2 * np, hipMemcpyHostToDevice, s));
        if (c.d1) {
            HIPCHK(hipMemcpyAsync(h->in_d1.p, c.d1, sizeof(double) * np, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(h->in_d2.p, c.d2, sizeof(double) * np, hipMemcpyHostToDevice, s));
        }
    }
    if (models) HIPCHK(hipMemcpyAsync(h->fm_models.p, *models, sizeof(Model) * b, hipMemcpyHostToDevice, s));
    if (with_scores) HIPCHK(hipMemcpyAsync(h->pr_scores.p, *scores, sizeof(double) * np, hipMemcpyHostToDevice, s));
    c.x1 = h->in_x1.as<double>(); c.x2 = h->in_x2.as<double>();
    if (c.d1) { c.d1 = h->in_d1.as<double>(); c.d2 = h->in_d2.as<double>(); }
    if (models) *models = h->fm_models.as<Model>();
    if (with_scores) *scores = h->pr_scores.as<double>();
    return MDRP_OK;
}

// the start-model scores of a refine call are host outputs whatever mem_space says: a buffer of the handle, copied back by finish_blocking
struct StartOutputs {
    double *score_host;
    int32_t *inl_host;
    double *score_dev = nullptr;
    int32_t *inl_dev = nullptr;
};
static int stage_start_outputs(mdrp_handle *h, int batch, StartOutputs &so) {
    if (!so.score_host && !so.inl_host) return MDRP_OK;
    const size_t off_inl = sizeof(double) * (size_t)batch;
    if (int rc = h->fm_init.ensure(off_inl + sizeof(int32_t) * (size_t)batch + 16)) return rc;
    so.score_dev = so.score_host ? h->fm_init.as<double>() : nullptr;
    so.inl_dev = so.inl_host ? reinterpret_cast<int32_t *>(h->fm_init.as<unsigned char>() + off_inl) : nullptr;
    return MDRP_OK;
}

// The end of every blocking call: a host call's mask (its planes, in a budgets call) back from the handle's, the start-model scores of a refine call,
// then the records (which waits for the handle's stream).
static int finish_blocking(mdrp_handle *h, const EstimateCall &c, bool use_host, mdrp_result *out, uint8_t *inlier_mask, const StartOutputs *start) {
    const size_t np = (size_t)c.batch * c.n_max, b = (size_t)c.batch;
    hipStream_t s = h->stream;
    hipError_t e = hipSuccess;
    if (use_host && inlier_mask && np > 0)
        e = hipMemcpyAsync(inlier_mask, (c.budgets ? h->bmask : h->mask).p, np * (c.budgets ? c.n_budgets : 1), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && start && start->score_dev && b > 0) e = hipMemcpyAsync(start->score_host, start->score_dev, sizeof(double) * b, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && start && start->inl_dev && b > 0) e = hipMemcpyAsync(start->inl_host, start->inl_dev, sizeof(int32_t) * b, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) { g_err = start ? "copy of the masks or start-model scores failed" : "copy of the inlier masks failed"; return MDRP_ERR_HIP; }
    return c.budgets ? budget_results_locked(h, out, c.n_budgets, c.batch, hipMemcpyDeviceToHost) : fetch_results_locked(h, out, c.batch);
}

// a blocking call behind its refusals: stage the host buffers, run the device-resident path (`run`, on the repointed call), finish
template <typename Run>
static int run_blocking(mdrp_handle *h, EstimateCall &c, int mem_space, const Model **models, const double **scores, mdrp_result *out, uint8_t *inlier_mask,
                        StartOutputs *start, Run run) {
    MDRP_ENTER(h);
    const bool use_host = mem_space == MDRP_MEM_HOST;
    int rc;
    if (use_host && (rc = stage_host_call(h, c, models, scores))) return rc;
    if (start && (rc = stage_start_outputs(h, c.batch, *start))) return rc;
    c.mask_dev = use_host ? nullptr : inlier_mask; // (host call: the handle's mask, copied back by finish_blocking)
    if ((rc = run())) return rc;
    return finish_blocking(h, c, use_host, out, inlier_mask, start);
}

// mdrp_estimate_batch[_budgets]: host buffers take the sliced front instead of stage_host_call (the copies are issued by run_pass, slice by slice on the
// handle's copy stream, beside the first kernels of the slices before them: Pass::host_front); the end is the shared one
static int estimate_batch_blocking(mdrp_handle *h, EstimateCall &c, int mem_space, mdrp_result *out, uint8_t *inlier_mask) {
    MDRP_ENTER(h);
    const size_t np = (size_t)c.batch * c.n_max;
    const bool use_host = mem_space == MDRP_MEM_HOST;
    int rc;
    HostSrc hsrc{};
    if (use_host) {
        if ((rc = h->in_x1.ensure(sizeof(double) * 2 * np + 16)) || (rc = h->in_x2.ensure(sizeof(double) * 2 * np + 16)) ||
            (rc = h->in_d1.ensure(sizeof(double) * np + 16)) || (rc = h->in_d2.ensure(sizeof(double) * np + 16)))
            return rc;
        const bool depths = c.d1 && c.d2;
        hsrc = HostSrc{c.x1, c.x2, depths ? c.d1 : nullptr, depths ? c.d2 : nullptr};
        if (depths) { c.d1 = h->in_d1.as<double>(); c.d2 = h->in_d2.as<double>(); }
        c.x1 = h->in_x1.as<double>(); c.x2 = h->in_x2.as<double>();
        c.host = &hsrc;
    }
    c.mask_dev = use_host ? nullptr : inlier_mask;
    if ((rc = estimate_device(h, c))) return rc;
    return finish_blocking(h, c, use_host, out, inlier_mask, nullptr);
}

// ---- refine and verify caller-supplied models
// What refine_device and refine_classic_device share in front of their one kernel: the handle's counters and result buffers, the per-call parameters
// in one block, the record / state buffers, the mask (the caller's or the handle's), the run parameters, and the events around the launch.
struct RefineStage {
    const int32_t *nper, *table_of;
    const CamDev *cam1, *cam2;
    uint8_t *mask;
    RunParams rp;
    hipEvent_t f0, f1; // reported as the final refinement's time (mdrp_stats::final_ms / final_launches)
};
// returns MDRP_OK with st.mask == nullptr for an empty batch (nothing to launch)
static int refine_stage(mdrp_handle *h, const EstimateCall &c, int est_shift, RefineStage &st) {
    const int kind = c.kind, batch = c.batch, n_max = c.n_max;
    const mdrp_ransac_opt *ro = c.ro;
    const mdrp_bundle_opt *bo = c.bo;
    hipStream_t s = h->stream;
    st.mask = nullptr;
    h->begin_call(batch, 0);
    int rc;
    if ((rc = h->results.ensure(sizeof(ResultDev) * std::max(batch, 1))) || (rc = h->lm_stats.ensure(LM_STATS_BYTES))) return rc;
    HIPCHK(hipMemsetAsync(h->lm_stats.p, 0, LM_STATS_BYTES, s));
    if (batch == 0) return MDRP_OK;
    const size_t b = (size_t)batch, n = (size_t)n_max;
    const bool mono = kind <= MDRP_VARYING_FOCAL;
    // per-call parameters in one block: cameras 1 | cameras 2 | table of pair (zeros: there are no sample tables) | n per pair.  Staged in pageable
    // memory (the copy has left it when hipMemcpyAsync returns): an asynchronous call may be followed by the next one before the stream has drained
    const size_t off_cam2 = sizeof(CamDev) * b, off_tof = 2 * sizeof(CamDev) * b, off_nper = off_tof + sizeof(int32_t) * b, bytes = off_nper + sizeof(int32_t) * b;
    std::vector<unsigned char> params(bytes, 0);
    if (kind == MDRP_CALIB || kind == MDRP_RELPOSE_5PT || kind == MDRP_SHARED_6PT) { // MDRP_SHARED_6PT reads the principal point from cam1 only: cam2 may be NULL there
        std::memcpy(params.data(), c.cam1, sizeof(CamDev) * b);
        std::memcpy(params.data() + off_cam2, c.cam2 ? c.cam2 : c.cam1, sizeof(CamDev) * b);
    }
    int32_t *nper = reinterpret_cast<int32_t *>(params.data() + off_nper);
    for (int i = 0; i < batch; ++i) nper[i] = c.n_per_pair ? c.n_per_pair[i] : n_max;
    if ((rc = h->pts.ensure(sizeof(double) * PT_STRIDE * b * std::max<size_t>(n, 1))) || (mono && (rc = h->dep.ensure(sizeof(double) * 2 * b * n))) ||
        (rc = h->st.ensure(sizeof(PairState) * b)) || (rc = h->params.ensure(bytes)))
        return rc;
    uint8_t *mask = c.mask_dev;
    if (!mask) { // (the baselines' kernel uses the mask as its LO's subset mask as well)
        if ((rc = h->mask.ensure(b * std::max(n_max, 1)))) return rc;
        mask = h->mask.as<uint8_t>();
    }
    unsigned char *pd = h->params.as<unsigned char>();
    HIPCHK(hipMemcpyAsync(pd, params.data(), bytes, hipMemcpyHostToDevice, s));
    st.nper = reinterpret_cast<const int32_t *>(pd + off_nper); st.table_of = reinterpret_cast<const int32_t *>(pd + off_tof);
    st.cam1 = reinterpret_cast<const CamDev *>(pd); st.cam2 = reinterpret_cast<const CamDev *>(pd + off_cam2);
    RunParams &rp = st.rp;
    std::memset(&rp, 0, sizeof rp);
    rp.kind = kind; rp.solver = solver_for(kind, est_shift); rp.est_shift = est_shift;
    rp.batch = batch; rp.n_max = n_max;
    if (!mono) { rp.mps = sched::model_slots(kind); rp.sample_sz = sched::sample_size(kind); } // (kc_prep: a pair of fewer records than the sample size is empty)
    rp.weight_sampson = (mono && ro->monodepth_weight_sampson > 0.0f) ? (double)ro->monodepth_weight_sampson : 0.0;
    rp.final_max_it = (int)std::min<uint64_t>(bo->max_iterations, 1u << 30); rp.final_loss = bo->loss_type;
    rp.grad_tol = bo->gradient_tol; rp.step_tol = bo->step_tol; rp.lambda0 = bo->initial_lambda;
    rp.lambda_min = bo->min_lambda; rp.lambda_max = bo->max_lambda;
    if ((rc = get_events(h, &st.f0, &st.f1, 3))) return rc;
    st.mask = mask;
    return MDRP_OK;
}

// k_prep as the estimators launch it (no MFMA fragments, no sample tables, score_initial = 0), then ONE launch of k_from_model on the handle's stream:
// nothing else of a pass is allocated or run.  Pointers are device memory, `models` included; init_* may be null.
static int refine_device(mdrp_handle *h, const EstimateCall &c, const Model *models, int stages, double *init_score, int32_t *init_inl) {
    hipStream_t s = h->stream;
    const int kind = c.kind, batch = c.batch, n_max = c.n_max;
    const int est_shift = (kind == MDRP_CALIB && c.ro->monodepth_estimate_shift) ? 1 : 0;
    RefineStage st;
    if (int rc = refine_stage(h, c, est_shift, st)) return rc;
    if (!st.mask) return MDRP_OK;
    const RunParams &rp = st.rp;
    uint8_t *mask = st.mask;
    hipLaunchKernelGGL(k_prep, dim3(batch), dim3(256), 0, s, rp, c.x1, c.x2, c.d1, c.d2, st.nper, st.table_of, st.cam1, st.cam2,
                       c.ro->max_epipolar_error, c.ro->max_reproj_error, c.bo->loss_scale, h->pts.as<double>(), h->dep.as<double>(), h->st.as<PairState>(),
                       (uint4 *)nullptr);
    HIPCHK(hipEventRecord(st.f0, s));
    const size_t smem = lm_final_list_bytes(n_max);
    const int stride = lm_list_stride(n_max), midx = lm_mask_index_on(n_max);
#define MDRP_FROM_MODEL_LAUNCH(K, S)                                                                                                                      \
    hipLaunchKernelGGL((k_from_model<K, S>), dim3(batch), dim3(FROM_MODEL_THREADS), smem, s, rp, (const PairState *)h->st.as<PairState>(),                \
                       (const double *)h->pts.as<double>(), (const double *)h->dep.as<double>(), models, stages, mask, h->results.as<ResultDev>(), init_score, \
                       init_inl, stride, midx, h->lm_stats.as<unsigned long long>() + 2)
    if (kind == MDRP_CALIB && est_shift) MDRP_FROM_MODEL_LAUNCH(0, true);
    else if (kind == MDRP_CALIB) MDRP_FROM_MODEL_LAUNCH(0, false);
    else if (kind == MDRP_SHARED_FOCAL) MDRP_FROM_MODEL_LAUNCH(1, false);
    else MDRP_FROM_MODEL_LAUNCH(2, false);
#undef MDRP_FROM_MODEL_LAUNCH
    HIPCHK(hipEventRecord(st.f1, s));
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

// the baselines: kc_prep as the estimators launch it, then ONE launch of kc_from_model (refine_device's shape, through the same refine_stage)
static int refine_classic_device(mdrp_handle *h, const EstimateCall &c, const Model *models, int stages, double *init_score, int32_t *init_inl) {
    hipStream_t s = h->stream;
    const int kind = c.kind, batch = c.batch, n_max = c.n_max;
    RefineStage st;
    if (int rc = refine_stage(h, c, 0, st)) return rc;
    if (!st.mask) return MDRP_OK;
    const RunParams &rp = st.rp;
    uint8_t *mask = st.mask;
    hipLaunchKernelGGL(kc_prep, dim3(batch), dim3(256), 0, s, rp, c.x1, c.x2, st.nper, st.table_of, st.cam1, st.cam2, c.ro->max_epipolar_error, c.bo->loss_scale,
                       h->pts.as<double>(), h->st.as<PairState>(), (uint4 *)nullptr);
    HIPCHK(hipEventRecord(st.f0, s));
    const int stride = lm_list_stride(n_max);
    const size_t smem = (size_t)2 * stride * sizeof(uint16_t);
#define MDRP_KC_FROM_MODEL_LAUNCH(CK)                                                                                                                   \
    hipLaunchKernelGGL((kc_from_model<CK>), dim3(batch), dim3(CLASSIC_MODEL_THREADS), smem, s, rp, (const PairState *)h->st.as<PairState>(),            \
                       (const double *)h->pts.as<double>(), models, stages, mask, h->results.as<ResultDev>(), init_score, init_inl, stride)
    if (kind == MDRP_RELPOSE_5PT) MDRP_KC_FROM_MODEL_LAUNCH(CLASSIC_RELPOSE);
    else if (kind == MDRP_SHARED_6PT) MDRP_KC_FROM_MODEL_LAUNCH(CLASSIC_SHARED);
    else MDRP_KC_FROM_MODEL_LAUNCH(CLASSIC_FUND);
#undef MDRP_KC_FROM_MODEL_LAUNCH
    HIPCHK(hipEventRecord(st.f1, s));
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

// ---- estimate in match-score order
// n per pair on the device for the ranking kernels (pr_nper), and scores -> order (pr_order, or `order_dev`) on the handle's stream
static int rank_device(mdrp_handle *h, const double *scores_dev, int batch, int n_max, const int32_t *n_per_pair, int32_t *order_dev) {
    hipStream_t s = h->stream;
    std::vector<int32_t> n_host(batch);
    for (int i = 0; i < batch; ++i) n_host[i] = n_per_pair ? n_per_pair[i] : n_max;
    if (int rc = h->pr_nper.ensure(sizeof(int32_t) * (size_t)batch)) return rc;
    HIPCHK(hipMemcpyAsync(h->pr_nper.p, n_host.data(), sizeof(int32_t) * (size_t)batch, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_rank, dim3(batch), dim3(RANK_THREADS), 0, s, scores_dev, (const int32_t *)h->pr_nper.as<int32_t>(), n_max, order_dev);
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

// All pointers device memory; scores_dev null: the records are in quality order already.  Ranks, gathers into the handle's ordered copies (allocated
// before estimate_device takes the pass budget from the free memory), runs the unchanged estimator with the progressive sampler on them, and
// scatters the mask into the caller's order: the call's mask_dev, or the handle's mask where that is null.  d1 / d2 null: a baseline call.
static int ranked_device(mdrp_handle *h, EstimateCall c, const double *scores_dev) {
    const RankedRun rr(*c.ro);
    rr.apply(c);
    const int batch = c.batch, n_max = c.n_max;
    const size_t np = (size_t)batch * n_max;
    if (!scores_dev || np == 0) return estimate_device(h, c);
    hipStream_t s = h->stream;
    int rc;
    const bool depths = c.kind <= MDRP_VARYING_FOCAL; // (a baseline call: no ordered copies of the depths)
    if ((rc = h->pr_x1.ensure(sizeof(double) * 2 * np)) || (rc = h->pr_x2.ensure(sizeof(double) * 2 * np)) || (depths && (rc = h->pr_d1.ensure(sizeof(double) * np))) ||
        (depths && (rc = h->pr_d2.ensure(sizeof(double) * np))) || (rc = h->pr_order.ensure(sizeof(int32_t) * np)) || (rc = h->pr_mask.ensure(np)))
        return rc;
    double *d1o = depths ? h->pr_d1.as<double>() : nullptr, *d2o = depths ? h->pr_d2.as<double>() : nullptr;
    uint8_t *mask = c.mask_dev;
    if (!mask) {
        if ((rc = h->mask.ensure(np))) return rc;
        mask = h->mask.as<uint8_t>();
    }
    int32_t *order = h->pr_order.as<int32_t>();
    if ((rc = rank_device(h, scores_dev, batch, n_max, c.n_per_pair, order))) return rc;
    const dim3 rgrid((unsigned)batch, (unsigned)((n_max + 255) / 256));
    const int32_t *nper = h->pr_nper.as<int32_t>();
    hipLaunchKernelGGL(k_rank_gather, rgrid, dim3(256), 0, s, (const int32_t *)order, nper, n_max, c.x1, c.x2, c.d1, c.d2, h->pr_x1.as<double>(), h->pr_x2.as<double>(),
                       d1o, d2o);
    HIPCHK(hipGetLastError());
    c.x1 = h->pr_x1.as<double>(); c.x2 = h->pr_x2.as<double>(); c.d1 = d1o; c.d2 = d2o;
    c.mask_dev = h->pr_mask.as<uint8_t>();
    if ((rc = estimate_device(h, c))) return rc;
    hipLaunchKernelGGL(k_rank_scatter, rgrid, dim3(256), 0, s, (const int32_t *)order, nper, n_max, (const uint8_t *)h->pr_mask.as<uint8_t>(), mask);
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

// ---- the device front ends (mdrp_frontend.h): the monodepth estimators' (keypoints, matches and depth maps) and the baselines'
// (include/mdrp_classic_frontend.h; DESIGN.md 7g: no depth maps, no d1 / d2), over four descriptors
static int check_matches(const mdrp_matches *mm, int batch) {
    const char *why = nullptr;
    if (!mm || batch < 0) why = "invalid argument";
    else if ((mm->kp_type != MDRP_F32 && mm->kp_type != MDRP_F64) || (mm->depth_type != MDRP_F32 && mm->depth_type != MDRP_F64)) why = "kp_type / depth_type must be MDRP_F32 or MDRP_F64";
    else if (mm->filter != MDRP_FILTER_BOTH_INF && mm->filter != MDRP_FILTER_FINITE) why = "unknown filter";
    else if (mm->k1 < 0 || mm->k2 < 0 || mm->m_max < 0 || mm->h1 < 0 || mm->w1 < 0 || mm->h2 < 0 || mm->w2 < 0) why = "negative size";
    else if (batch > 0 && mm->m_max > 0 &&
             (!mm->matches || (mm->k1 > 0 && !mm->kp1) || (mm->k2 > 0 && !mm->kp2) || (mm->h1 > 0 && mm->w1 > 0 && !mm->depth1) ||
              (mm->h2 > 0 && mm->w2 > 0 && !mm->depth2)))
        why = "NULL keypoints, matches or depth map";
    if (why) { g_err = std::string("mdrp_matches: ") + why; return MDRP_ERR_INVALID; }
    return MDRP_OK;
}

static int check_image_pairs(const mdrp_image_pairs *ip, int batch) {
    const char *why = nullptr;
    if (!ip || batch < 0) why = "invalid argument";
    else if ((ip->kp_type != MDRP_F32 && ip->kp_type != MDRP_F64) || (ip->depth_type != MDRP_F32 && ip->depth_type != MDRP_F64)) why = "kp_type / depth_type must be MDRP_F32 or MDRP_F64";
    else if (ip->filter != MDRP_FILTER_BOTH_INF && ip->filter != MDRP_FILTER_FINITE) why = "unknown filter";
    else if (ip->k_max < 0 || ip->m_max < 0 || ip->h_max < 0 || ip->w_max < 0 || ip->n_images < 0) why = "negative size";
    else if (batch > 0 && ip->m_max > 0 && (!ip->pairs || !ip->matches)) why = "NULL pairs or matches";
    else if (ip->n_images > 0 && ip->k_max > 0 && !ip->kp) why = "NULL keypoints";
    else if (ip->n_images > 0 && ip->h_max > 0 && ip->w_max > 0 && !ip->depth) why = "NULL depth maps";
    if (why) { g_err = std::string("mdrp_image_pairs: ") + why; return MDRP_ERR_INVALID; }
    return MDRP_OK;
}

// check_matches / check_image_pairs without the depth clauses
static int check_point_matches(const mdrp_point_matches *pm, int batch) {
    const char *why = nullptr;
    if (!pm || batch < 0) why = "invalid argument";
    else if (pm->kp_type != MDRP_F32 && pm->kp_type != MDRP_F64) why = "kp_type must be MDRP_F32 or MDRP_F64";
    else if (pm->k1 < 0 || pm->k2 < 0 || pm->m_max < 0) why = "negative size";
    else if (batch > 0 && pm->m_max > 0 && (!pm->matches || (pm->k1 > 0 && !pm->kp1) || (pm->k2 > 0 && !pm->kp2))) why = "NULL keypoints or matches";
    if (why) { g_err = std::string("mdrp_point_matches: ") + why; return MDRP_ERR_INVALID; }
    return MDRP_OK;
}

static int check_point_image_pairs(const mdrp_point_image_pairs *pp, int batch) {
    const char *why = nullptr;
    if (!pp || batch < 0) why = "invalid argument";
    else if (pp->kp_type != MDRP_F32 && pp->kp_type != MDRP_F64) why = "kp_type must be MDRP_F32 or MDRP_F64";
    else if (pp->k_max < 0 || pp->m_max < 0 || pp->n_images < 0) why = "negative size";
    else if (batch > 0 && pp->m_max > 0 && (!pp->pairs || !pp->matches)) why = "NULL pairs or matches";
    else if (pp->n_images > 0 && pp->k_max > 0 && !pp->kp) why = "NULL keypoints";
    if (why) { g_err = std::string("mdrp_point_image_pairs: ") + why; return MDRP_ERR_INVALID; }
    return MDRP_OK;
}

static int check_score_type(const void *scores, int score_type) {
    if (!scores || score_type == MDRP_F32 || score_type == MDRP_F64) return MDRP_OK;
    g_err = "score_type must be MDRP_F32 or MDRP_F64";
    return MDRP_ERR_INVALID;
}

static int check_front_end_kind(int kind, bool depths, const char *who) {
    const int first = depths ? MDRP_CALIB : MDRP_RELPOSE_5PT;
    if (kind >= first && kind <= first + 2) return MDRP_OK;
    g_err = std::string(who) + (depths ? ": only the monodepth estimators (kind 0..2) take depth maps"
                                       : ": only the baselines (MDRP_RELPOSE_5PT, MDRP_SHARED_6PT, MDRP_FUNDAMENTAL_7PT); the monodepth estimators need depth maps: mdrp_estimate_matches_async takes them");
    return MDRP_ERR_INVALID;
}

// a descriptor's element types as the arguments of a generic lambda: every gather kernel is launched from one place per form (plain | ranked)
template <typename F> static void with_kp_type(int kp_type, F f) {
    if (kp_type == MDRP_F32) f(float{});
    else f(double{});
}
template <typename F> static void with_kp_depth_types(int kp_type, int depth_type, F f) {
    with_kp_type(kp_type, [&](auto kt) {
        if (depth_type == MDRP_F32) f(kt, float{});
        else f(kt, double{});
    });
}

// The gathers on the handle's stream, one per descriptor (which has passed its check); n_dev: [batch] on the device.  With scores ([batch][m_max] of
// score_type, device memory) the ranked kernel: the kept rows at their ranks; the handle's key scratch has been sized (ensure_key_scratch).
// The baselines' have no depths: d1 / d2 are not looked at.
static int gather_device(mdrp_handle *h, const mdrp_matches *mm, int batch, double *x1, double *x2, double *d1, double *d2, int32_t *slot, int32_t *n_dev,
                         const void *scores, int score_type) {
    if (batch == 0) return MDRP_OK;
    with_kp_depth_types(mm->kp_type, mm->depth_type, [&](auto kt, auto dt) {
        using KT = decltype(kt);
        using DT = decltype(dt);
        const KT *kp1 = (const KT *)mm->kp1, *kp2 = (const KT *)mm->kp2;
        const DT *dm1 = (const DT *)mm->depth1, *dm2 = (const DT *)mm->depth2;
        if (scores)
            hipLaunchKernelGGL((k_gather_ranked<KT, DT>), dim3(batch), dim3(FE_THREADS), 0, h->stream, kp1, kp2, mm->k1, mm->k2, mm->matches, mm->m_max, dm1, dm2,
                               mm->h1, mm->w1, mm->h2, mm->w2, mm->center1, mm->center2, mm->filter, scores, score_type, h->fe_key.as<uint64_t>(), x1, x2, d1, d2,
                               slot, n_dev);
        else
            hipLaunchKernelGGL((k_gather<KT, DT>), dim3(batch), dim3(FE_THREADS), 0, h->stream, kp1, kp2, mm->k1, mm->k2, mm->matches, mm->m_max, dm1, dm2, mm->h1,
                               mm->w1, mm->h2, mm->w2, mm->center1, mm->center2, mm->filter, x1, x2, d1, d2, slot, n_dev);
    });
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

// (the three per-image and depth-free descriptors: no rows, and pairs may be NULL - the counts are all there is to write)
static int gather_nothing(mdrp_handle *h, int batch, int32_t *n_dev) {
    HIPCHK(hipMemsetAsync(n_dev, 0, sizeof(int32_t) * batch, h->stream));
    return MDRP_OK;
}

static int gather_images_device(mdrp_handle *h, const mdrp_image_pairs *ip, int batch, double *x1, double *x2, double *d1, double *d2, int32_t *slot,
                                int32_t *n_dev, const void *scores, int score_type) {
    if (batch == 0) return MDRP_OK;
    if (ip->m_max == 0) return gather_nothing(h, batch, n_dev);
    with_kp_depth_types(ip->kp_type, ip->depth_type, [&](auto kt, auto dt) {
        using KT = decltype(kt);
        using DT = decltype(dt);
        if (scores)
            hipLaunchKernelGGL((k_gather_images_ranked<KT, DT>), dim3(batch), dim3(FE_THREADS), 0, h->stream, (const KT *)ip->kp, ip->kp_count, ip->k_max,
                               (const DT *)ip->depth, ip->size, ip->h_max, ip->w_max, ip->center, ip->n_images, ip->pairs, ip->matches, ip->m_max, ip->filter, scores,
                               score_type, h->fe_key.as<uint64_t>(), x1, x2, d1, d2, slot, n_dev);
        else
            hipLaunchKernelGGL((k_gather_images<KT, DT>), dim3(batch), dim3(FE_THREADS), 0, h->stream, (const KT *)ip->kp, ip->kp_count, ip->k_max, (const DT *)ip->depth,
                               ip->size, ip->h_max, ip->w_max, ip->center, ip->n_images, ip->pairs, ip->matches, ip->m_max, ip->filter, x1, x2, d1, d2, slot, n_dev);
    });
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

static int gather_points_device(mdrp_handle *h, const mdrp_point_matches *pm, int batch, double *x1, double *x2, double *, double *, int32_t *slot, int32_t *n_dev,
                                const void *scores, int score_type) {
    if (batch == 0) return MDRP_OK;
    if (pm->m_max == 0) return gather_nothing(h, batch, n_dev);
    with_kp_type(pm->kp_type, [&](auto kt) {
        using KT = decltype(kt);
        if (scores)
            hipLaunchKernelGGL((k_gather_points_ranked<KT>), dim3(batch), dim3(FE_THREADS), 0, h->stream, (const KT *)pm->kp1, (const KT *)pm->kp2, pm->k1, pm->k2,
                               pm->matches, pm->m_max, pm->center1, pm->center2, scores, score_type, h->fe_key.as<uint64_t>(), x1, x2, slot, n_dev);
        else
            hipLaunchKernelGGL((k_gather_points<KT>), dim3(batch), dim3(FE_THREADS), 0, h->stream, (const KT *)pm->kp1, (const KT *)pm->kp2, pm->k1, pm->k2, pm->matches,
                               pm->m_max, pm->center1, pm->center2, x1, x2, slot, n_dev);
    });
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

static int gather_point_images_device(mdrp_handle *h, const mdrp_point_image_pairs *pp, int batch, double *x1, double *x2, double *, double *, int32_t *slot,
                                      int32_t *n_dev, const void *scores, int score_type) {
    if (batch == 0) return MDRP_OK;
    if (pp->m_max == 0) return gather_nothing(h, batch, n_dev);
    with_kp_type(pp->kp_type, [&](auto kt) {
        using KT = decltype(kt);
        if (scores)
            hipLaunchKernelGGL((k_gather_points_images_ranked<KT>), dim3(batch), dim3(FE_THREADS), 0, h->stream, (const KT *)pp->kp, pp->kp_count, pp->k_max, pp->center,
                               pp->n_images, pp->pairs, pp->matches, pp->m_max, scores, score_type, h->fe_key.as<uint64_t>(), x1, x2, slot, n_dev);
        else
            hipLaunchKernelGGL((k_gather_points_images<KT>), dim3(batch), dim3(FE_THREADS), 0, h->stream, (const KT *)pp->kp, pp->kp_count, pp->k_max, pp->center,
                               pp->n_images, pp->pairs, pp->matches, pp->m_max, x1, x2, slot, n_dev);
    });
    HIPCHK(hipGetLastError());
    return MDRP_OK;
}

// a front end: whether it has depths, its descriptor's check, its gather
template <typename Desc> struct FrontEnd {
    bool depths;
    int (*check)(const Desc *, int);
    int (*gather)(mdrp_handle *, const Desc *, int, double *, double *, double *, double *, int32_t *, int32_t *, const void *, int);
};
static const FrontEnd<mdrp_matches> FE_MATCHES{true, check_matches, gather_device};
static const FrontEnd<mdrp_image_pairs> FE_IMAGE_PAIRS{true, check_image_pairs, gather_images_device};
static const FrontEnd<mdrp_point_matches> FE_POINT_MATCHES{false, check_point_matches, gather_points_device};
static const FrontEnd<mdrp_point_image_pairs> FE_POINT_IMAGE_PAIRS{false, check_point_image_pairs, gather_point_images_device};

// the ranked gathers' key scratch (one key per match row), a buffer of the handle
static int ensure_key_scratch(mdrp_handle *h, int batch, int m_max) { return h->fe_key.ensure(sizeof(uint64_t) * (size_t)batch * m_max + 16); }

// the counts of the last gather into the handle's pinned block: the one stream synchronisation of the front end
static int fetch_counts(mdrp_handle *h, int batch) {
    if (batch == 0) return MDRP_OK;
    if ((size_t)batch > h->fe_n_host_cap) {
        h->fe_n_host.reset();
        h->fe_n_host_cap = 0;
        HIPCHK(hipHostMalloc((void **)&h->fe_n_host.v, sizeof(int32_t) * ((size_t)batch + batch / 8 + 64), hipHostMallocDefault));
        h->fe_n_host_cap = (size_t)batch + batch / 8 + 64;
    }
    HIPCHK(hipMemcpyAsync(h->fe_n_host, h->fe_n.p, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MDRP_OK;
}

// the handle's gather buffers for batch pairs of m_max rows (depths false: the baselines' front end leaves fe_d1 / fe_d2 as they are)
static int ensure_gather_buffers(mdrp_handle *h, int batch, int m_max, bool depths) {
    const size_t rows = (size_t)batch * m_max;
    int rc;
    if ((rc = h->fe_x1.ensure(sizeof(double) * 2 * rows + 16)) || (rc = h->fe_x2.ensure(sizeof(double) * 2 * rows + 16)) ||
        (depths && ((rc = h->fe_d1.ensure(sizeof(double) * rows + 16)) || (rc = h->fe_d2.ensure(sizeof(double) * rows + 16)))) ||
        (rc = h->fe_slot.ensure(sizeof(int32_t) * rows + 16)) || (rc = h->fe_n.ensure(sizeof(int32_t) * std::max(batch, 1))))
        return rc;
    return MDRP_OK;
}

// the gather alone into the caller's buffers: the counts cross to n_host behind one stream synchronisation
template <typename Desc>
static int gather_alone(mdrp_handle *h, const FrontEnd<Desc> &fe, const Desc *desc, const void *scores_dev, int score_type, int batch, double *x1, double *x2, double *d1,
                        double *d2, int32_t *slot, int32_t *n_host, const char *who) {
    if (!h) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (int rc = fe.check(desc, batch)) return rc;
    if (int rc = check_score_type(scores_dev, score_type)) return rc;
    if (batch > 0 && (!n_host || (desc->m_max > 0 && (!x1 || !x2 || (fe.depths && (!d1 || !d2)) || !slot)))) { g_err = std::string(who) + ": NULL output"; return MDRP_ERR_INVALID; }
    MDRP_ENTER(h);
    int rc;
    if ((rc = h->fe_n.ensure(sizeof(int32_t) * std::max(batch, 1))) || (scores_dev && (rc = ensure_key_scratch(h, batch, desc->m_max)))) return rc;
    if ((rc = fe.gather(h, desc, batch, x1, x2, d1, d2, slot, h->fe_n.as<int32_t>(), scores_dev, score_type))) return rc;
    if ((rc = fetch_counts(h, batch))) return rc;
    if (batch > 0) std::memcpy(n_host, h->fe_n_host, sizeof(int32_t) * batch);
    return MDRP_OK;
}

// Front end + estimator.  Refusals (the estimator's own among them, on the options as it will see them: nothing is queued for a call it refuses); the gather
// into the handle's buffers; the counts (one stream synchronisation); the resident estimator on the gathered buffers with the handle's own inlier mask
// (by slot); that mask back onto the match rows.  ranked: the gathered buffers are in quality order and the progressive sampler draws from them.
template <typename Desc>
static int estimate_front(mdrp_handle *h, const FrontEnd<Desc> &fe, int kind, const Desc *desc, const void *scores_dev, int score_type, bool ranked, int batch,
                          const mdrp_camera *cam1, const mdrp_camera *cam2, const mdrp_ransac_opt *ropt, const mdrp_bundle_opt *bopt, uint8_t *match_mask_dev,
                          int32_t *n_used_host, const char *who) {
    if (!h || !ropt || !bopt) { g_err = "invalid argument"; return MDRP_ERR_INVALID; }
    if (int rc = check_front_end_kind(kind, fe.depths, who)) return rc;
    if (int rc = fe.check(desc, batch)) return rc;
    if (int rc = check_score_type(scores_dev, score_type)) return rc;
    static const double own = 0.0; // the depths are buffers of the handle, not yet sized: `own` stands for them in the refusals
    const int m_max = desc->m_max;
    EstimateCall c = call_of(kind, nullptr, nullptr, fe.depths ? &own : nullptr, fe.depths ? &own : nullptr, batch, m_max, nullptr, cam1, cam2, ropt, bopt);
    if (int rc = refusals_as_run(h, c, ranked)) return rc;
    MDRP_ENTER(h);
    const size_t rows = (size_t)batch * m_max;
    int rc;
    if ((rc = ensure_gather_buffers(h, batch, m_max, fe.depths)) || (scores_dev && (rc = ensure_key_scratch(h, batch, m_max)))) return rc;
    c.x1 = h->fe_x1.as<double>(); c.x2 = h->fe_x2.as<double>();
    c.d1 = fe.depths ? h->fe_d1.as<double>() : nullptr; c.d2 = fe.depths ? h->fe_d2.as<double>() : nullptr;
    if ((rc = fe.gather(h, desc, batch, h->fe_x1.as<double>(), h->fe_x2.as<double>(), h->fe_d1.as<double>(), h->fe_d2.as<double>(), h->fe_slot.as<int32_t>(),
                        h->fe_n.as<int32_t>(), scores_dev, score_type)))
        return rc;
    if ((rc = fetch_counts(h, batch))) return rc;
    c.n_per_pair = batch > 0 ? h->fe_n_host.v : nullptr;
    const RankedRun rr(*ropt);
    if (ranked) rr.apply(c);
    if ((rc = estimate_device(h, c))) return rc;
    if (match_mask_dev && rows > 0) {
        hipLaunchKernelGGL(k_match_mask, dim3((unsigned)((rows + FE_THREADS - 1) / FE_THREADS)), dim3(FE_THREADS), 0, h->stream, h->fe_slot.as<int32_t>(),
                           h->mask.as<uint8_t>(), m_max, rows, match_mask_dev);
        HIPCHK(hipGetLastError());
    }
    if (n_used_host && batch > 0) std::memcpy(n_used_host, h->fe_n_host, sizeof(int32_t) * batch);
    return MDRP_OK;
}
