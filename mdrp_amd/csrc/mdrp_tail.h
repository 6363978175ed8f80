// mdrp_tail.h — everything that runs once RANSAC has a candidate model: the LO plan, the walk and its checkpoints, the fused tail's
// protocol, and the stage bodies — LO queue, final, from a caller's model, prior — as __device__ templates over an estimator family's descriptor
// (MonoFam here, ClassicFam in mdrp_classic.h).  The kernels (k_lo / k_final here, k_from_model, k_prior, kc_lo, kc_final, kc_from_model, kc_prior in
// their headers) are wrappers: they declare and initialise the LDS state and call a body.  A body never asks which family it serves; a difference
// between the families is a member of the descriptor or stays in the wrapper.  One stage keeps two bodies: the final pair is final_pair<Fam> for
// the baselines and final_pair_mono for the mono-depth family (the reason stands there); both go through the same helpers.
#pragma once
#include "mdrp_kernels.h"

namespace mdrp {

// ------------------------------------------------------------------------------------------------ LO
// Persistent workgroups pop (pair, trigger) items; each refines the triggering minimal model (refine_model
// @0x4fa550/@0x4fad60/@0x4fb0a0: 25 it, TRUNCATED) and rescoring it.
#define MDRP_LM_MINWAVES 2
// LO work plan of one chunk: the triggers the chunk's scan appended to each pair's list, as a prefix sum over the pairs.
// The plan is frozen when it is built (begin/end per pair), so k_lo of this chunk can run on a second stream while the
// next chunk's scan keeps appending triggers — the LO of the first, short chunk (most of a run's LO work: records fall
// fast at the start) hides behind the second chunk's sweep instead of leaving the chip to the tail of a launch whose
// single problems take ~1 ms on one wavefront.
// (Measured and dropped: longest-first ordering by inlier count — no change.  XCD-affine queues, pair p on XCD p mod 8: 2.8x less HBM
// fetch, same time in round 2; as contiguous eighths of the plan with stealing (lo_take, round 4) 2-5 % of k_lo: the LO is bound by
// instruction issue at 1-2 waves/SIMD, not by bandwidth or order.)
// plan layout: prefix[B+1] | begin[B] | end[B] | total
MDRP_GLOBAL __launch_bounds__(PLAN_THREADS) void k_lo_plan(int batch, const PairState *__restrict__ st, const int32_t *__restrict__ prev_plan /*or null*/,
                                                          int32_t *__restrict__ plan) {
    __shared__ int s_w[PLAN_THREADS / 64 + 1];
    int32_t *prefix = plan, *begin = plan + batch + 1, *end = begin + batch;
    const int32_t *prev_end = prev_plan ? prev_plan + 2 * (size_t)batch + 1 : nullptr;
    int run = 0;
    for (int p0 = 0; p0 < batch; p0 += PLAN_THREADS) {
        const int p = p0 + threadIdx.x;
        int b = 0, e = 0;
        if (p < batch) { b = prev_end ? prev_end[p] : 0; e = st[p].n_triggers; if (e < b) e = b; }
        int tot;
        const int ex = plan_block_scan(e - b, tot, s_w);
        if (p < batch) { prefix[p] = run + ex; begin[p] = b; end[p] = e; }
        run += tot;
    }
    if (threadIdx.x == 0) { prefix[batch] = run; plan[3 * (size_t)batch + 1] = run; }
}

// ------------------------------------------------------------------------------------------------ walk
// One lane per pair replays score_models<> / ransac<> bookkeeping (@0x22ebc0, @0x22f030) over the ordered triggers
// and applies the dynamic stopping rule.
// lo_plans / n_plans / lo_cap: the LM engine refines at most lo_cap triggers of a chunk per pass (its problem table is sized
// before anyone knows how many triggers the scans will find); if a chunk found more, nothing is replayed yet — the flag
// n_active[1] tells the host to run the remaining passes and launch the walk again.
// Replay of one pair (one lane).  Returns true if the pair has stopped; otherwise `need` = iterations it still certainly needs.
// COHERENT: the LO results in the triggers were written by other workgroups of the SAME launch (fused tail): they are read with
// agent-scope atomic loads, which neither the compiler (restrict / invariance reasoning) nor the scalar cache can serve from
// anything older than the acquire that preceded the call.
__device__ __forceinline__ double coherent_f64(const double *p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// (uint64_t) of a double as the reference's x86-64 build computes it (comisd against 2^63; cvttsd2si; the high half via d - 2^63 and a flipped top
// bit): what the dynamic iteration bound becomes when it leaves the range — success_prob = 1 gives +inf -> 0 (the search ends right after
// min_iterations), NaN (success_prob > 1) gives 2^63 (never), a negative bound wraps.  v_cvt saturates instead.  tests/golden/edge_options_ref.npz
__device__ __forceinline__ uint64_t f64_to_u64_x86(double d) {
    const double t63 = 9223372036854775808.0;
    if (d >= t63) {
        const double e = d - t63;
        return (e < t63 ? (uint64_t)(int64_t)e : 0x8000000000000000ull) ^ 0x8000000000000000ull;
    }
    return d >= -t63 ? (uint64_t)(int64_t)d : 0x8000000000000000ull; // (NaN fails both comparisons: cvttsd2si's "integer indefinite")
}
// ransac<>'s dynamic iteration bound behind a refinement, from the inlier ratio of the best model so far (walk_pair, prior_stage)
__device__ __forceinline__ uint64_t dyn_max_iter_of(const RunParams &rp, double inlier_ratio) {
    if (inlier_ratio >= 0.9999) return rp.min_iterations;
    if (inlier_ratio <= 0.0001) return rp.max_iterations;
    // pow(ratio, sample size) of the reference: x * x * x for 3 (pinned against the binary), libm pow otherwise
    const double prob_outlier = 1.0 - (rp.sample_sz == 3 ? inlier_ratio * inlier_ratio * inlier_ratio : pow(inlier_ratio, (double)rp.sample_sz));
    return f64_to_u64_x86(ceil(rp.log_prob_missing / log(prob_outlier) * rp.dyn_mult));
}
// SNAP (a budgets call's k_walk_ckpt only): the pair's state as it is when `iterations` reaches budget K_c — or the pair stops, if that
// comes first — is copied into ck[c * ck_plane], with iterations = min(K_c, stop) and active = 0: what a run with max_iterations = K_c leaves behind,
// since nothing but `it` changes between two triggers and the stop test cannot fire differently before K_c.  The copy is taken BEFORE a trigger at an
// absolute iteration >= K_c is executed and before `it` passes K_c in a trigger-free stretch, at a stop or at the end of the super-chunk.
template <bool COHERENT = false, bool SNAP = false>
__device__ bool walk_pair(const RunParams &rp, PairState &ps, const Model *__restrict__ models, const Trigger *trig /*of this pair*/,
                          size_t slot_base, uint64_t &need, const uint64_t *__restrict__ budgets = nullptr, int n_budgets = 0,
                          PairState *__restrict__ ck = nullptr /*this pair's row of checkpoint 0*/, size_t ck_plane = 0) {
    need = 0;
    if (!ps.active) return true;
    // max_iterations = 0: the reference's loop head ends the search before a sample is drawn (ransac<>: iterations < max_iterations) — no record, no
    // LO; the closing LO then runs on the reset identity model (tests/golden/edge_options_ref.npz)
    if (rp.max_iterations == 0) { ps.iterations = 0; ps.active = 0; return true; }
    const uint64_t c0 = rp.chunk_start, c1 = rp.chunk_start + (uint64_t)rp.super_len;
    uint64_t it = c0; // iterations completed so far
    bool stopped = false;
    int nc = 0; // SNAP: the first checkpoint still open (those up to the super-chunk's start were filled by the super-chunks before)
    if constexpr (SNAP) while (nc < n_budgets && budgets[nc] <= c0) ++nc;
    // SNAP: every open checkpoint with K_c <= upto takes the state as it is, at min(K_c, at) iterations
    auto snap = [&](uint64_t upto, uint64_t at) {
        if constexpr (SNAP)
            for (; nc < n_budgets && budgets[nc] <= upto; ++nc) {
                PairState &d = ck[(size_t)nc * ck_plane];
                d = ps;
                d.iterations = budgets[nc] < at ? budgets[nc] : at;
                d.active = 0;
            }
    };
    // stop test applied after each completed iteration: it >= max -> stop; it > min && it > dyn -> stop
    // (+ 1 saturates: a bound of 2^64 - 1 — the reference's (uint64_t) of a dynamic bound in (-2, -1], dyn_num_trials_mult < 0 — is never exceeded, and
    // the sum must not wrap to 0 and end the run at min_iterations + 1; max_iterations then caps the saturated value, and it >= max_iterations stops)
    auto next_of = [](uint64_t v) -> uint64_t { return v == ~0ull ? v : v + 1; };
    auto first_stop = [&](uint64_t lo /*first candidate value of it*/) -> uint64_t {
        uint64_t s = lo;
        if (s < next_of(ps.dyn_max_iter)) s = next_of(ps.dyn_max_iter);
        if (s < next_of(rp.min_iterations)) s = next_of(rp.min_iterations);
        if (s > rp.max_iterations) s = rp.max_iterations;
        if (lo > s) s = lo;
        return s;
    };
    for (int k = 0; k < ps.n_triggers && !stopped; ++k) {
        const Trigger &tr = trig[k];
        const uint64_t ti = c0 + tr.iter; // absolute index of the triggering iteration
        // iterations it .. ti-1 complete without bookkeeping changes; would the loop stop at a value in (it, ti] ?
        if (ti > it) {
            const uint64_t s = first_stop(it + 1);
            if (s <= ti) { it = s; stopped = true; break; }
        }
        snap(ti, ~0ull); // (iterations it .. ti - 1 changed nothing: the state at K_c <= ti is this one)
        // execute iteration ti
        if (tr.k_min >= 0 && tr.score_min < ps.model_score) {
            ps.model_score = tr.score_min;
            ps.best = models[slot_base + (size_t)tr.iter * rp.mps + tr.k_min];
            ps.num_inliers = (uint64_t)tr.cnt_min;
        }
        ps.refinements++;
        const double ref_score = COHERENT ? coherent_f64(&tr.ref_score) : tr.ref_score;
        if (ref_score < ps.model_score) {
            ps.model_score = ref_score;
            if (COHERENT) {
                ps.num_inliers = (uint64_t)__hip_atomic_load(&tr.ref_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                static_assert(sizeof(Model) % 8 == 0, "Model is copied as doubles");
                const double *src = reinterpret_cast<const double *>(&tr.refined);
                double *dst = reinterpret_cast<double *>(&ps.best);
#pragma unroll
                for (int q = 0; q < (int)(sizeof(Model) / 8); ++q) dst[q] = coherent_f64(src + q);
            } else {
                ps.num_inliers = (uint64_t)tr.ref_cnt;
                ps.best = tr.refined;
            }
        }
        ps.inlier_ratio = (double)ps.num_inliers / (double)ps.n;
        ps.dyn_max_iter = dyn_max_iter_of(rp, ps.inlier_ratio);
        it = ti + 1;
        if (it >= rp.max_iterations || (it > rp.min_iterations && it > ps.dyn_max_iter)) { stopped = true; break; }
    }
    if (!stopped) {
        // remaining iterations of the chunk
        if (c1 > it) {
            const uint64_t s = first_stop(it + 1);
            if (s <= c1) { it = s; stopped = true; } else it = c1;
        }
    }
    snap(stopped ? ~0ull : c1, stopped ? it : ~0ull); // stopped: every checkpoint still open reports the stopped state
    ps.iterations = it;
    if (stopped) { ps.active = 0; return true; }
    need = first_stop(it + 1) - it; // iterations still certainly needed with the current dyn_max_iter
    return false;
}

MDRP_GLOBAL void k_walk(RunParams rp, PairState *__restrict__ st, const Model *__restrict__ models, const Trigger *__restrict__ triggers,
                       int trig_cap, int32_t *__restrict__ n_active, unsigned long long *__restrict__ max_needed,
                       const int32_t *__restrict__ lo_plans, int n_plans, int plan_stride, int lo_cap) {
    const int pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= rp.batch) return;
    for (int c = 0; c < n_plans; ++c)
        if (lo_plans[(size_t)c * plan_stride + 3 * (size_t)rp.batch + 1] > lo_cap) {
            if (pair == 0) n_active[1] = 1;
            return;
        }
    PairState &ps = st[pair];
    if (!ps.active) return;
    uint64_t need;
    if (!walk_pair<false>(rp, ps, models, triggers + (size_t)pair * trig_cap, (size_t)pair * rp.slot_stride, need)) {
        atomicAdd(n_active, 1);
        atomicMax(max_needed, (unsigned long long)need);
    }
}

// The walk of a budgets call: k_walk that also fills the pair's checkpoints, ckpt[c * rp.batch + pair] for budget c.  Pairs that never
// iterate (fewer correspondences than a sample) report the state k_prep gave them at every budget.
constexpr int WALK_CKPT_THREADS = 64; // (the launch bound lets a lane hold a whole PairState in registers while it copies it: no scratch)
MDRP_GLOBAL __launch_bounds__(WALK_CKPT_THREADS) void k_walk_ckpt(RunParams rp, PairState *__restrict__ st, const Model *__restrict__ models, const Trigger *__restrict__ triggers,
                            int trig_cap, int32_t *__restrict__ n_active, unsigned long long *__restrict__ max_needed,
                            const uint64_t *__restrict__ budgets, int n_budgets, PairState *__restrict__ ckpt) {
    const int pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= rp.batch) return;
    PairState &ps = st[pair];
    if (!ps.active) {
        if (rp.chunk_start == 0)
            for (int c = 0; c < n_budgets; ++c) ckpt[(size_t)c * rp.batch + pair] = ps;
        return;
    }
    uint64_t need;
    if (!walk_pair<false, true>(rp, ps, models, triggers + (size_t)pair * trig_cap, (size_t)pair * rp.slot_stride, need, budgets, n_budgets,
                                ckpt + pair, (size_t)rp.batch)) {
        atomicAdd(n_active, 1);
        atomicMax(max_needed, (unsigned long long)need);
    }
}

// Only distinct states are refined: `refinements` grows whenever a pair's state changes, so two checkpoints of a pair with equal `refinements` differ
// in `iterations` at most.  One workgroup: per pair, the first checkpoint of every run of equal `refinements` goes on `list` (problems c * batch +
// pair, ordered by pair, then budget; the unused tail is -1: surplus workgroups of the final launch leave at once), and rep[c * batch + pair] names
// the problem whose result every checkpoint shares.
MDRP_GLOBAL __launch_bounds__(PLAN_THREADS) void k_ckpt_plan(int batch, int n_budgets, const PairState *__restrict__ ckpt, int32_t *__restrict__ list,
                                                            int32_t *__restrict__ rep) {
    __shared__ int s_w[PLAN_THREADS / 64 + 1];
    int run = 0;
    for (int p0 = 0; p0 < batch; p0 += PLAN_THREADS) {
        const int p = p0 + threadIdx.x;
        int kept = 0;
        if (p < batch)
            for (int c = 0; c < n_budgets; ++c)
                kept += c == 0 || ckpt[(size_t)c * batch + p].refinements != ckpt[(size_t)(c - 1) * batch + p].refinements;
        int tot;
        const int ex = plan_block_scan(kept, tot, s_w);
        if (p < batch) {
            int w = run + ex, r = 0;
            for (int c = 0; c < n_budgets; ++c) {
                const int e = c * batch + p;
                if (c == 0 || ckpt[e].refinements != ckpt[e - batch].refinements) { r = e; list[w++] = e; }
                rep[e] = r;
            }
        }
        run += tot;
    }
    for (int i = run + threadIdx.x; i < n_budgets * batch; i += PLAN_THREADS) list[i] = -1;
}

// Fused tail (the LAST LO launch of a run whose end is known): the workgroup that refines the last open trigger of a
// pair replays the pair (walk_pair, instead of a k_walk launch) and appends it to `ready`.  When the LO queue is empty - its last
// problems are in flight, most wavefront slots are already free - k_gate lets the final refinements start on another stream:
// workgroup i of k_final takes the i-th ready pair.  The few whose pair is not ready yet wait for problems that resident LO
// workgroups hold (nobody needs their slots: the queue is empty), so the wait cannot block anything.
struct FuseTail {
    int32_t *done_cnt;   // [batch] refined triggers of this launch per pair (zeroed)
    int32_t *ready;      // [batch] pairs in the order they became ready (-1 = not yet)
    int32_t *ctl;        // [0] entries of `ready`, [1] LO workgroups that have started (their trigger-less pairs are published)   (zeroed)
    PairState *st;       // mutable alias of the pair states (only the walking lane writes)
};
// one lane: returns when every workgroup of the LO launch has started and every problem has been taken from its queue - from then
// on whatever a final refinement may wait for is in the hands of a resident workgroup.
// Both this wait and the final refinements' wait for their pair are BOUNDED (`ticks` of the 100 MHz clock): where kernels of
// different streams cannot run side by side (rocprofv3 --pmc serialises dispatches, debuggers do) the LO launch may be stuck behind
// the very kernels that wait for it.  Then the gate gives up, the final workgroups give up and leave their pairs undone, the LO
// launch runs, and the ordinary k_final pass behind it (`skip`) refines what is left: slower, never stuck.
// LO queue with XCD affinity.  The problems of a launch are sorted by pair (k_lo_plan) and every LM sweep re-reads its pair's records
// (96 KB at N = 2000, 240 KB at N = 5000; ~18 sweeps per problem): with one queue the ~5 problems of a pair run on five different XCDs and
// every sweep comes over the fabric.  Eight queues, one per XCD, each over a contiguous eighth of the plan: an XCD's wavefronts work on ~46
// consecutive pairs at a time and the problems of a pair share its L2.  The LO is bound by instruction issue, not by the memory side
// (DESIGN.md 4): this buys 2-5 % of k_lo, no more.  A workgroup whose own queue is empty takes from the others (the tail stays balanced);
// which problem runs where changes nothing but speed.  `head` counts the tickets handed out (k_gate waits on it); xheads == null: one queue.
constexpr int LO_XCD_STRIDE = 16; // int32 between two queue heads (their own 64-byte blocks)
__device__ __forceinline__ int lo_xcc_id() {
    int x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    return x & 7;
}
__device__ __forceinline__ int lo_take(int32_t *__restrict__ head, int32_t *__restrict__ xheads, int total) {
    if (!xheads) return atomicAdd(head, 1);
    const int x = lo_xcc_id();
    for (int k = 0; k < 8; ++k) {
        const int y = (x + k) & 7;
        const int b = (int)((long long)total * y / 8), len = (int)((long long)total * (y + 1) / 8) - b;
        if (len <= 0 || __hip_atomic_load(xheads + y * LO_XCD_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= len) continue;
        const int t = atomicAdd(xheads + y * LO_XCD_STRIDE, 1);
        if (t < len) { atomicAdd(head, 1); return b + t; }
    }
    return total;
}

MDRP_GLOBAL void k_gate(const int32_t *__restrict__ lo_head, const int32_t *__restrict__ plan_total, const int32_t *__restrict__ ctl, int lo_blocks,
                       unsigned long long ticks, unsigned long long *__restrict__ timeouts /*[0] gate, [1] final waits: mdrp_stats.fuse_*_timeouts*/) {
    const int total = *plan_total;
    const unsigned long long t0 = wall_clock64();
    bool open = false;
    while (!(open = __hip_atomic_load(ctl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= lo_blocks &&
                    __hip_atomic_load(lo_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= total) && wall_clock64() - t0 < ticks)
        __builtin_amdgcn_s_sleep(64);
    if (!open && timeouts) atomicAdd(timeouts, 1ull);
}
__device__ __forceinline__ void fuse_publish(const FuseTail &fz, const RunParams &rp, int pair, const Model *__restrict__ models,
                                             const Trigger *__restrict__ triggers, int trig_cap) {
    uint64_t need;
    walk_pair<true>(rp, fz.st[pair], models, triggers + (size_t)pair * trig_cap, (size_t)pair * rp.slot_stride, need);
    __threadfence();
    const int t = atomicAdd(fz.ctl, 1);
    __hip_atomic_store(fz.ready + t, pair, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------ what the stage bodies share
// ransac<>'s LO (refine_model): 25 iterations, always TRUNCATED at the pair's threshold
__device__ __forceinline__ LmOpt lo_opt(const PairState &ps) {
    LmOpt o;
    o.max_it = 25; o.loss = 1; o.loss_scale = ps.lo_loss_scale;
    o.grad_tol = 1e-10; o.step_tol = 1e-8; o.lambda0 = 1e-3; o.lambda_min = 1e-10; o.lambda_max = 1e10;
    return o;
}
// the estimators' inlier-only refinement: the caller's BundleOptions
__device__ __forceinline__ LmOpt final_opt(const RunParams &rp, const PairState &ps, int loss) {
    LmOpt o;
    o.max_it = rp.final_max_it; o.loss = loss; o.loss_scale = ps.final_loss_scale;
    o.grad_tol = rp.grad_tol; o.step_tol = rp.step_tol; o.lambda0 = rp.lambda0; o.lambda_min = rp.lambda_min; o.lambda_max = rp.lambda_max;
    return o;
}
// A pair state (and a caller's model, bit for bit) is read ONCE, with vector loads, into LDS: its fields are re-readable there, so that nothing but
// the model under refinement is live across an LM.  Volatile: in a fused tail the state was written DURING this launch (by the LO workgroup that
// replayed the pair); a kernel that never writes `st` may otherwise fetch st[pair] through the scalar cache, which an acquire does not invalidate
// and which can hold the cache line that the previous pair's last field shares with this pair's head from BEFORE the replay.  The caller's next
// barrier publishes the copy.
constexpr int PAIR_STATE_WORDS = (int)((sizeof(PairState) + 3) / 4), MODEL_WORDS = (int)(sizeof(Model) / 4);
template <int T>
__device__ __forceinline__ void stage_pair(unsigned int *s_ps, const PairState *ps, unsigned int *s_m0 = nullptr, const Model *m0 = nullptr) {
    const volatile unsigned int *src = reinterpret_cast<const volatile unsigned int *>(ps);
    for (int i = threadIdx.x; i < (int)(sizeof(PairState) / 4); i += T) s_ps[i] = src[i];
    if (s_m0) {
        const volatile unsigned int *msrc = reinterpret_cast<const volatile unsigned int *>(m0);
        for (int i = threadIdx.x; i < MODEL_WORDS; i += T) s_m0[i] = msrc[i];
    }
}

// The estimator family behind a stage body (lo_queue, final_pair, from_model_stage, prior_stage below) is a small descriptor:
//   T, MIN_N              lanes per problem; the smallest n that is searched
//   MIN_INLIERS           the inlier-only refinement runs with MORE inliers than this
//   Lds                   the family's LDS state (its wrapper kernel declares and initialises it)
//   score(m, row, ps, score, count, mask)     exact MSAC score of a model; with a mask it ends with a barrier (the mask is read by other lanes next)
//   lo(m, row, ps, subset)                    ransac<>'s refine_model under lo_opt
//   lo_counts(m)                              from a caller's model: whether the LO stage runs and counts for this start model
//   refine_inliers(m, row, ps, mask, o)       the inlier-only refinement under the caller's options
//   start(m0, ps, space) / finish(x, ps)      a caller's model into the estimator's units / a result back to the caller's
//   end_problem()                             after a problem's last barrier, lane 0
// `row` is the pair's row of the record arrays.  The mono-depth family (KIND, SHIFT) is here, the 5- / 6- / 7-point baselines' in mdrp_classic.h.
constexpr int STAGE_LO = 1, STAGE_INLIERS = 2; // MDRP_STAGE_* of include/mdrp.h
template <int KIND, bool SHIFT, int T_>
struct MonoFam {
    static constexpr int T = T_, MIN_N = 3;
    static constexpr int MIN_INLIERS = KIND == 2 ? 7 : 3; // calibrated (@0x224434) and shared-focal (@0x2235e6) wrappers: 3; varying-focal (@0x223d16): 7
    using Lds = LmShared;
    const RunParams &rp;
    const double *pts, *dep;
    Lds &sh;
    __device__ __forceinline__ const double *pp(int row) const { return pts + (size_t)row * rp.n_max * PT_STRIDE; }
    __device__ __forceinline__ const double *dd(int row) const { return dep + (size_t)row * rp.n_max * 2; }
    __device__ __forceinline__ void score(const Model &m, int row, const PairState &ps, double &sc, int &cn, uint8_t *__restrict__ mask) const {
        block_score<T>(KIND, m, pp(row), ps.n, ps.sq_thr, sh.scratch, sc, cn, mask);
        if (mask) __syncthreads();
    }
    // all records.  A NaN model — the reference's P3P, k_solve — has a NaN cost: no step can be accepted, it comes back as it is
    __device__ __forceinline__ void lo(Model &m, int row, const PairState &ps, uint8_t * /*subset*/) const {
        if (m.q[0] == m.q[0]) lm_refine<KIND, SHIFT, T, 1>(m, pp(row), dd(row), ps.n, nullptr, ps.scale_reproj, rp.weight_sampson, lo_opt(ps), sh);
    }
    __device__ __forceinline__ bool lo_counts(const Model &m) const { return m.q[0] == m.q[0]; } // a NaN model is scored and verified, never refined
    // the loss is read at run time (o.loss)
    __device__ __forceinline__ void refine_inliers(Model &m, int row, const PairState &ps, const uint8_t *__restrict__ mask, const LmOpt &o) const {
        lm_refine<KIND, SHIFT, T, -1>(m, pp(row), dd(row), ps.n, mask, ps.scale_reproj, rp.weight_sampson, o, sh);
    }
    // the focal kinds work on coordinates divided by the pair's normalisation scale
    __device__ __forceinline__ Model start(const Model *__restrict__ m0, const PairState &ps, int /*space*/) const {
        Model x = *m0;
        if (KIND != 0) { x.f1 /= ps.norm; x.f2 /= ps.norm; }
        return x;
    }
    __device__ __forceinline__ void finish(Model &x, const PairState &ps) const {
        if (KIND != 0) { x.f1 *= ps.norm; x.f2 *= ps.norm; }
    }
    __device__ __forceinline__ void end_problem() const { lm_flush_stats(sh); }
};
// the wrappers' initialisation of the mono-depth LDS state (lane 0)
__device__ __forceinline__ void lm_shared_init(LmShared &sh, uint16_t *list, int list_stride, int mask_index, unsigned long long *stats, const double *logtab) {
    sh.list = list; sh.stride = list_stride; sh.midx = mask_index; sh.stats = stats; sh.ev[0] = 0; sh.ev[1] = 0; sh.logtab = logtab;
}

// ------------------------------------------------------------------------------------------------ LO queue
// LO of item w of the launch's plan (refine_model + score_model of the refined model), by the whole workgroup
template <class Fam>
__device__ void lo_problem(const Fam &fam, const RunParams &rp, const PairState *__restrict__ st, const Model *__restrict__ models,
                           Trigger *__restrict__ triggers, int trig_cap, const int32_t *__restrict__ plan, int w, uint8_t *__restrict__ subset,
                           const FuseTail &fz) {
    const int32_t *prefix = plan, *begin = plan + rp.batch + 1, *end = begin + rp.batch;
    const int pair = plan_find(prefix, rp.batch, w);
    const int pos = begin[pair] + (w - prefix[pair]);
    const PairState &ps = st[pair];
    Trigger &tr = triggers[(size_t)pair * trig_cap + pos];
    const size_t slot_base = (size_t)pair * rp.slot_stride;
    Model m = models[slot_base + (size_t)tr.iter * rp.mps + tr.k_ref];
    fam.lo(m, pair, ps, subset);
    double sc;
    int cn;
    fam.score(m, pair, ps, sc, cn, nullptr);
    if (threadIdx.x == 0) {
        tr.refined = m; tr.ref_score = sc; tr.ref_cnt = cn;
        fam.end_problem();
        if (fz.ready) {
            __threadfence(); // this trigger's results before the count
            if (atomicAdd(fz.done_cnt + pair, 1) + 1 == end[pair] - begin[pair]) {
                __threadfence(); // the other triggers' results (written on other CUs / XCDs) before the replay reads them
                fuse_publish(fz, rp, pair, models, triggers, trig_cap);
            }
        }
    }
}

// The persistent loop of an LO launch: the workgroup takes items of the plan until the queues are empty.  `subset`: this workgroup's row for the
// family's LO mask, or null.
template <class Fam>
__device__ __forceinline__ void lo_queue(const Fam &fam, const RunParams &rp, const PairState *__restrict__ st, const Model *__restrict__ models,
                                         Trigger *__restrict__ triggers, int trig_cap, const int32_t *__restrict__ plan, int32_t *__restrict__ head,
                                         int32_t *__restrict__ xheads, uint8_t *__restrict__ subset, const FuseTail &fz, int &s_item) {
    const int total = plan[3 * (size_t)rp.batch + 1];
    if (fz.ready && threadIdx.x == 0) { // pairs without a trigger in this launch are ready as they are (earlier LO launches have ended: stream order)
        const int32_t *begin = plan + rp.batch + 1, *end = begin + rp.batch;
        for (int p = blockIdx.x; p < rp.batch; p += gridDim.x)
            if (end[p] == begin[p]) fuse_publish(fz, rp, p, models, triggers, trig_cap);
        atomicAdd(fz.ctl + 1, 1);
    }
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) s_item = lo_take(head, xheads, total);
        __syncthreads();
        const int w = s_item;
        if (w >= total) break;
        lo_problem(fam, rp, st, models, triggers, trig_cap, plan, w, subset, fz);
    }
}

template <int KIND, bool SHIFT, int T>
__global__ __launch_bounds__(T, MDRP_LM_MINWAVES) void k_lo(RunParams rp, const PairState *__restrict__ st, const double *__restrict__ pts,
                                                   const double *__restrict__ dep, const Model *__restrict__ models,
                                                   Trigger *__restrict__ triggers, int trig_cap, const int32_t *__restrict__ plan,
                                                   int32_t *__restrict__ head /*zeroed*/, int32_t *__restrict__ xheads /*zeroed, or null: lo_take*/,
                                                   int list_stride, unsigned long long *__restrict__ lm_stats, FuseTail fz /*ready == null: off*/) {
    extern __shared__ uint16_t lm_dyn_list[];
    __shared__ LmShared sh;
    __shared__ int s_item;
    if (threadIdx.x == 0) lm_shared_init(sh, lm_dyn_list, list_stride, 0, lm_stats, nullptr);
    __syncthreads();
    lo_queue(MonoFam<KIND, SHIFT, T>{rp, pts, dep, sh}, rp, st, models, triggers, trig_cap, plan, head, xheads, nullptr, fz, s_item);
}

// ------------------------------------------------------------------------------------------------ final
// ransac<> tail (@0x22f1d0-0x22f295) + get_inliers (@0x4f7a10/@0x4f77f0) + the estimator's inlier-only refinement
// (@0x2247c3 / @0x223815) + focal un-normalisation.
struct ResultDev {
    Model model;
    uint64_t refinements, iterations, num_inliers;
    double inlier_ratio, model_score;
};

// the record of a pair as its state stands, but for what the final stage moves on: the model, the refinements and the inliers
__device__ __forceinline__ ResultDev result_of(const PairState &ps, const Model &model, uint64_t refinements, uint64_t num_inliers) {
    ResultDev res;
    res.model = model;
    res.refinements = refinements; res.iterations = ps.iterations; res.num_inliers = num_inliers;
    res.inlier_ratio = ps.inlier_ratio; res.model_score = ps.model_score;
    return res;
}

// Lane 0: the pair this workgroup refines, or -1 for none.  Fused tail (`ready`): the blockIdx-th pair to become ready, bounded wait (see k_gate).
// Otherwise pair blockIdx.x, unless `fin_done` marks it: the pass behind a fused tail refines only what that left undone.
__device__ __forceinline__ int final_take(const int32_t *__restrict__ ready, const int32_t *__restrict__ fin_done, unsigned long long ticks,
                                          unsigned long long *__restrict__ timeouts) {
    int p = blockIdx.x;
    if (ready) {
        const unsigned long long t0 = wall_clock64();
        // polled RELAXED, one acquire fence when the pair is there: an acquire LOAD is followed by an invalidate of the XCD's L2, and the few
        // hundred workgroups waiting here did that every microsecond while the last LO problems were still sweeping.  (Found with an experimental
        // queue-driven k_final whose idle workgroups polled the same way: the pairs still running took twice as long per iteration.)
        while ((p = __hip_atomic_load(ready + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < 0 && wall_clock64() - t0 < ticks)
            __builtin_amdgcn_s_sleep(16);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (p < 0 && timeouts) atomicAdd(timeouts, 1ull); // gave up: the pass behind the LO launch refines this pair (mdrp_stats.fuse_wait_timeouts)
        __threadfence(); // the replayed pair state (written on another CU / XCD) before anyone of this workgroup reads it
    } else if (fin_done && fin_done[p]) p = -1;
    return p;
}

// ransac<>'s tail for one pair: the last LO from the best model, adopted iff it scores better; get_inliers of the winner; the estimator's
// inlier-only refinement with the user's BundleOptions; back to the caller's units; the record.  Nothing but the model under refinement is live
// across an LM (`ps` is the LDS copy): the round-4 kernel carried `best`, `m`, `x` and the result record (100 VGPRs) through both refinements and
// spilled 201-449 VGPRs.
template <class Fam>
__device__ __forceinline__ void final_pair(const Fam &fam, const RunParams &rp, const PairState &ps, uint8_t *__restrict__ mask_all,
                                           ResultDev *__restrict__ results, int pair) {
    constexpr int T = Fam::T;
    const FinalRows row = final_rows(rp, pair);
    uint8_t *mask = mask_all + (size_t)row.out * rp.n_max;
    if (ps.n < Fam::MIN_N) {
        for (int i = threadIdx.x; i < rp.n_max; i += T) mask[i] = 0;
        if (threadIdx.x == 0) results[row.out] = result_of(ps, ps.best, ps.refinements, ps.num_inliers);
        return;
    }
    Model x = ps.best;
    fam.lo(x, row.rec, ps, mask); // (the output mask doubles as the LO's subset mask)  counted below whether or not an LM ran
    uint64_t num_inliers = ps.num_inliers;
    {
        double sc;
        int cn;
        fam.score(x, row.rec, ps, sc, cn, nullptr);
        if (sc < ps.model_score) num_inliers = (uint64_t)cn; // the refined model is adopted; score / ratio NOT updated (reference)
        else x = ps.best;                                    // (re-read: no second model is kept live across the LM)
        for (int i = ps.n + threadIdx.x; i < rp.n_max; i += T) mask[i] = 0;
        fam.score(x, row.rec, ps, sc, cn, mask);             // get_inliers of the winner
    }
    if (num_inliers > (uint64_t)Fam::MIN_INLIERS) fam.refine_inliers(x, row.rec, ps, mask, final_opt(rp, ps, rp.final_loss));
    fam.finish(x, ps);
    __syncthreads();
    if (threadIdx.x == 0) {
        results[row.out] = result_of(ps, x, ps.refinements + 1, num_inliers);
        fam.end_problem();
    }
}

// The mono-depth family's final pair keeps a body of its own, stated through the same helpers (lo_opt, final_opt, result_of).  With BOTH of its LM calls
// behind descriptor members the compiler pairs four a * b - c * d expressions of the inlined sweeps into FMAs the other way round (-ffp-contract=fast),
// and the records change in their last bits; either call alone does not.  Which source lines of the sweeps (lm_cost, lm_accumulate_point and
// its Jacobian rows, mdrp_kernels.h) the four belong to is not recorded: an attempt to lift this, e.g. with a local `#pragma clang fp contract` around them,
// starts by comparing the v_fma_f64 / v_mul_f64 sequences of the two k_final disassemblies.  FLOSS: the loss of the inlier-only refinement as a compile-time constant
// (rp.final_loss; -1 = read at run time): its sweeps carry no six-way loss switch.
template <int KIND, bool SHIFT, int T, int FLOSS>
__device__ __forceinline__ void final_pair_mono(const RunParams &rp, const PairState &ps, const double *__restrict__ pts, const double *__restrict__ dep,
                                           uint8_t *__restrict__ mask_all, ResultDev *__restrict__ results, int pair, LmShared &sh) {
    double *scratch = sh.scratch;
    const FinalRows row = final_rows(rp, pair);
    uint8_t *mask = mask_all + (size_t)row.out * rp.n_max;
    if (ps.n < 3) {
        for (int i = threadIdx.x; i < rp.n_max; i += T) mask[i] = 0;
        if (threadIdx.x == 0) {
            results[row.out] = result_of(ps, ps.best, ps.refinements, ps.num_inliers);
        }
        return;
    }
    const double *pp = pts + (size_t)row.rec * rp.n_max * PT_STRIDE;
    const double *dd = dep + (size_t)row.rec * rp.n_max * 2;
    // ransac<>'s last LO from the best model: 25 iterations, TRUNCATED, all records
    Model x = ps.best;
    {
        if (x.q[0] == x.q[0]) lm_refine<KIND, SHIFT, T, 1>(x, pp, dd, ps.n, nullptr, ps.scale_reproj, rp.weight_sampson, lo_opt(ps), sh); // (NaN model: lo_problem)
    }
    uint64_t num_inliers = ps.num_inliers;
    {
        double sc;
        int cn;
        block_score<T>(KIND, x, pp, ps.n, ps.sq_thr, scratch, sc, cn, nullptr);
        if (sc < ps.model_score) num_inliers = (uint64_t)cn; // the refined model is adopted; score / ratio NOT updated (reference)
        else x = ps.best;                                    // (re-read: no second model is kept live across the LM)
        for (int i = ps.n + threadIdx.x; i < rp.n_max; i += T) mask[i] = 0;
        block_score<T>(KIND, x, pp, ps.n, ps.sq_thr, scratch, sc, cn, mask); // get_inliers of the winner
        __syncthreads();
    }
    // the estimator's inlier-only refinement with the user's BundleOptions: with more than 3 inliers in the calibrated (@0x224434) and shared-focal
    // (@0x2235e6) wrappers, with more than 7 in the varying-focal one (@0x223d16)
    if (num_inliers > (KIND == 2 ? 7u : 3u)) {
        const LmOpt o = final_opt(rp, ps, FLOSS >= 0 ? FLOSS : rp.final_loss);
        lm_refine<KIND, SHIFT, T, FLOSS>(x, pp, dd, ps.n, mask, ps.scale_reproj, rp.weight_sampson, o, sh);
    }
    if (KIND != 0) { x.f1 *= ps.norm; x.f2 *= ps.norm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        results[row.out] = result_of(ps, x, ps.refinements + 1, num_inliers);
        if (rp.inl_stat) { // what this pair would have liked as the run's first chunk: ~6 outlier-free samples expected in it (first_chunk_wish)
            atomicAdd(&rp.inl_stat[0], first_chunk_wish((double)num_inliers / (double)ps.n, 3));
            atomicAdd(&rp.inl_stat[1], 1);
        }
        lm_flush_stats(sh);
    }
}

// A final launch's workgroup (k_final, kc_final): lane 0 takes the workgroup's pair (final_take), the pair state goes through LDS (stage_pair) fused or
// not — ONE call site of the body (round 4 compiled the 17 k-instruction body twice) — and a fused launch marks the pair done.
template <int KIND, bool SHIFT, int T, int FLOSS>
__global__ __launch_bounds__(T, MDRP_LM_MINWAVES) void k_final(RunParams rp, PairState *__restrict__ st, const double *__restrict__ pts,
                                                      const double *__restrict__ dep, uint8_t *__restrict__ mask_all,
                                                      ResultDev *__restrict__ results, int list_stride, int mask_index /*1: 3 * list_stride entries of dynamic LDS*/,
                                                      unsigned long long *__restrict__ lm_stats,
                                                      const int32_t *__restrict__ ready /*or null: pair = blockIdx.x*/,
                                                      int32_t *__restrict__ fin_done /*fused: set per refined pair; unfused: pairs to skip, or null*/,
                                                      unsigned long long ticks, unsigned long long *__restrict__ timeouts /*fused: expired bounded waits*/) {
    extern __shared__ uint16_t lm_dyn_list[];
    __shared__ LmShared sh;
    __shared__ int s_pair;
    __shared__ __attribute__((aligned(16))) unsigned int s_ps[PAIR_STATE_WORDS];
    __shared__ __attribute__((aligned(16))) double s_logtab[(FLOSS == 3 || FLOSS == 4 || FLOSS < 0) ? 2 * MDRP_LOGTAB_N : 2];
    constexpr bool use_logtab = FLOSS == 3 || FLOSS == 4 || FLOSS < 0;
    if (use_logtab) lm_logtab_load(s_logtab);
    if (threadIdx.x == 0) {
        lm_shared_init(sh, lm_dyn_list, list_stride, mask_index, lm_stats, use_logtab ? s_logtab : nullptr);
        s_pair = final_take(ready, fin_done, ticks, timeouts);
    }
    __syncthreads();
    if (s_pair < 0) return;
    stage_pair<T>(s_ps, st + s_pair);
    __syncthreads();
    final_pair_mono<KIND, SHIFT, T, FLOSS>(rp, *reinterpret_cast<const PairState *>(s_ps), pts, dep, mask_all, results, s_pair, sh);
    if (ready && threadIdx.x == 0) fin_done[s_pair] = 1;
}

// ------------------------------------------------------------------------------------------------ from a caller's model
// One workgroup per pair runs what the estimator runs from the moment RANSAC has picked its winner, from a model the CALLER hands in:
//   score the start model | LO, adopted iff it scores better, WITH its own score | get_inliers | inlier-only LM | record
// `ps` and `m0` are the LDS copies (stage_pair).  When no stage ran the record carries *m0 bit for bit (verification, a NaN model: no round trip
// through the estimator's units).
__device__ __forceinline__ void from_model_stats(ResultDev &res, int refinements, int count, double ratio, double score) {
    res.refinements = (uint64_t)refinements; res.iterations = 0; res.num_inliers = (uint64_t)count;
    res.inlier_ratio = ratio; res.model_score = score;
}
// the record of a pair without a search or without a model: zeroed stats, the model as it came, no inliers
template <int T>
__device__ __forceinline__ void from_model_empty(const RunParams &rp, int pair, const Model *m0, double score, uint8_t *__restrict__ mask_all,
                                                 ResultDev *__restrict__ results, double *__restrict__ initial_score, int32_t *__restrict__ initial_inliers) {
    uint8_t *mask = mask_all + (size_t)pair * rp.n_max;
    for (int i = threadIdx.x; i < rp.n_max; i += T) mask[i] = 0;
    if (threadIdx.x == 0) {
        ResultDev res;
        res.model = *m0;
        from_model_stats(res, 0, 0, 0.0, score);
        results[pair] = res;
        if (initial_score) initial_score[pair] = score;
        if (initial_inliers) initial_inliers[pair] = 0;
    }
}
template <class Fam>
__device__ __forceinline__ void from_model_stage(const Fam &fam, const RunParams &rp, const PairState &ps, const Model *m0, int pair, int stages,
                                                 uint8_t *__restrict__ mask_all, ResultDev *__restrict__ results,
                                                 double *__restrict__ initial_score /*[batch] or null*/, int32_t *__restrict__ initial_inliers /*[batch] or null*/) {
    constexpr int T = Fam::T;
    if (ps.n < Fam::MIN_N) { // (the prep kernel: n = 0 for a pair of fewer correspondences than a sample) the estimators' rule
        from_model_empty<T>(rp, pair, m0, DBL_MAX, mask_all, results, initial_score, initial_inliers);
        return;
    }
    uint8_t *mask = mask_all + (size_t)pair * rp.n_max;
    Model x = fam.start(m0, ps, 0);
    // the start model's own score: the estimator's exact sweep (a NaN model: no inliers, n * sq_thr)
    double score;
    int count;
    fam.score(x, pair, ps, score, count, nullptr);
    if (threadIdx.x == 0) {
        if (initial_score) initial_score[pair] = score;
        if (initial_inliers) initial_inliers[pair] = count;
    }
    int refinements = 0;
    if ((stages & STAGE_LO) && fam.lo_counts(x)) { // ransac<>'s LO, counted whether or not its LM ran
        fam.lo(x, pair, ps, mask); // (the output mask doubles as the LO's subset mask)
        ++refinements;
        double sc;
        int cn;
        fam.score(x, pair, ps, sc, cn, nullptr);
        if (sc < score) { score = sc; count = cn; } // adopted WITH its own score (the estimator's record keeps the old one)
        else x = fam.start(m0, ps, 0);             // (re-read: no second model is kept live across the LM)
    }
    {   // get_inliers of the model kept so far
        double sc;
        int cn;
        for (int i = ps.n + threadIdx.x; i < rp.n_max; i += T) mask[i] = 0;
        fam.score(x, pair, ps, sc, cn, mask);
    }
    if ((stages & STAGE_INLIERS) && count > Fam::MIN_INLIERS) {
        fam.refine_inliers(x, pair, ps, mask, final_opt(rp, ps, rp.final_loss));
        ++refinements;
    }
    fam.finish(x, ps);
    __syncthreads();
    if (threadIdx.x == 0) {
        ResultDev res;
        if (refinements) res.model = x;
        else res.model = *m0; // no stage ran (verification, a model the family's LO does not count): the caller's record, no round trip
        from_model_stats(res, refinements, count, (double)count / (double)ps.n, score);
        results[pair] = res;
        fam.end_problem();
    }
}

// ------------------------------------------------------------------------------------------------ prior
// One workgroup per pair, behind the prep kernel and before the first solver or sweep reads the pair states, puts the pair into the state ransac<>
// is in after it has scored and LO-refined an initial model that was NOT reset to the identity (score_initial_model with *best = the prior):
//   score the prior | records (best_min_cnt, best_min_score) | best model | LO, adopted iff it scores better | inlier ratio and dynamic iteration bound
// Not an iteration: `iterations` stays 0 and no stop test runs.  Pairs of fewer correspondences than a sample and pairs whose prior has a NaN q[0]
// (no prior) keep what the prep kernel gave them, RansacOptions::score_initial_model included; a pair WITH a prior ignores that switch.
// `ps` and `m0` are the LDS copies (stage_pair); `subset`: the pair's row for the family's LO mask, or null.
template <class Fam>
__device__ __forceinline__ void prior_stage(const Fam &fam, const RunParams &rp, PairState *__restrict__ st, const PairState &ps, const Model *m0,
                                            int pair, int space, uint8_t *__restrict__ subset) {
    if (ps.n < Fam::MIN_N || !(m0->q[0] == m0->q[0])) return; // (uniform: read from LDS)  no search / no prior: the prep kernel's state stands
    Model x = fam.start(m0, ps, space);
    // score_models<> on {prior} against the empty records (0 inliers, DBL_MAX)
    double s0;
    int c0;
    fam.score(x, pair, ps, s0, c0, nullptr);
    const bool more = c0 > 0, better = s0 < DBL_MAX;
    double score = DBL_MAX; // model_score of the run
    int count = 0;
    if (s0 < score) { score = s0; count = c0; }
    int refinements = 0;
    bool adopted = false;
    if (more || better) { // (neither: a NaN score — no record, no LO)
        fam.lo(x, pair, ps, subset);
        refinements = 1;
        double s1;
        int c1;
        fam.score(x, pair, ps, s1, c1, nullptr);
        if (s1 < score) { score = s1; count = c1; adopted = true; }
    }
    if (threadIdx.x == 0) {
        PairState &d = st[pair];
        // the LO never touches the records of the minimal models
        d.best_min_cnt = more ? (uint64_t)c0 : 0;
        d.best_min_score = better ? s0 : DBL_MAX;
        d.model_score = score;
        d.num_inliers = (uint64_t)count;
        d.best = adopted ? x : fam.start(m0, ps, space); // (*best = the prior from the start: it stays where nothing beats DBL_MAX)
        d.refinements = (uint64_t)refinements;
        const double ratio = refinements ? (double)count / (double)ps.n : 0.0;
        d.inlier_ratio = ratio;
        d.dyn_max_iter = refinements ? dyn_max_iter_of(rp, ratio) : rp.max_iterations;
        d.iterations = 0; // not an iteration
        fam.end_problem();
    }
}

// Budgets call (k_ckpt_plan): behind the final refinements every other checkpoint takes its representative's record and mask row, with its own `iterations`.  One workgroup
// per (budget, pair); rows as final_rows.  The last budget's results feed rp.inl_stat, as the final refinements of a call without budgets do.
constexpr int CKPT_FILL_THREADS = 256;
MDRP_GLOBAL __launch_bounds__(CKPT_FILL_THREADS) void k_ckpt_fill(RunParams rp, int n_budgets, const PairState *__restrict__ ckpt,
                                                                 const int32_t *__restrict__ rep, ResultDev *__restrict__ results,
                                                                 uint8_t *__restrict__ mask_all) {
    const int e = blockIdx.x, r = rep[e];
    const FinalRows dst = final_rows(rp, e), src = final_rows(rp, r);
    if (r != e) {
        const uint8_t *from = mask_all + (size_t)src.out * rp.n_max;
        uint8_t *to = mask_all + (size_t)dst.out * rp.n_max;
        for (int i = threadIdx.x; i < rp.n_max; i += CKPT_FILL_THREADS) to[i] = from[i];
    }
    if (threadIdx.x == 0) {
        ResultDev res = results[src.out];
        if (r != e) { res.iterations = ckpt[e].iterations; results[dst.out] = res; }
        if (rp.inl_stat && e / rp.ck_pairs == n_budgets - 1 && ckpt[e].n >= 3) {
            atomicAdd(&rp.inl_stat[0], first_chunk_wish((double)res.num_inliers / (double)ckpt[e].n, 3));
            atomicAdd(&rp.inl_stat[1], 1);
        }
    }
}

} // namespace mdrp
