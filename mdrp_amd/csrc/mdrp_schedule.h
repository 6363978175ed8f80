// mdrp_schedule.h — the host scheduler's decisions (mdrp_capi.hip: run_pass, estimate_device) as plain functions: how a run's iterations are
// cut into super-chunks and chunks, how pairs share sample tables and passes, and the defaults of the knobs that depend on the call's shape.
// Host-only C++17 with no device header and no look at the environment (the caller reads the knobs and hands them in), so that
// tests/hostmath/schedule_host.cpp pins every rule here without a GPU (tests/test_schedule_host.py).
#pragma once
#include "../../include/mdrp.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

namespace mdrp {
namespace sched {

constexpr int NC_MAX = 8; // chunks of a super-chunk

inline int model_slots(int kind) { return kind == MDRP_RELPOSE_5PT ? 12 : (kind == MDRP_SHARED_6PT ? 16 : 4); } // model slots per sample
inline int sample_size(int kind) { return kind == MDRP_RELPOSE_5PT ? 5 : (kind == MDRP_SHARED_6PT ? 6 : (kind == MDRP_FUNDAMENTAL_7PT ? 7 : 3)); }

// iterations that certainly run: the reference cannot stop before min_iterations + 1 (or max_iterations)
inline uint64_t certain_iterations(uint64_t max_iterations, uint64_t min_iterations) {
    return max_iterations == 0 ? 1 : std::min<uint64_t>(max_iterations, min_iterations + 1);
}
// iterations a pass's scratch holds at once: the longest super-chunk
inline int chunk_capacity(uint64_t max_iterations, uint64_t min_iterations) {
    const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(max_iterations, 1), std::max<uint64_t>(min_iterations + 1, 4096));
    return (int)std::min<uint64_t>(cap, 16384);
}

// leading chunk lengths of a run's first super-chunk; the last chunk takes the rest
struct Lead {
    int n = 0;
    uint64_t len[NC_MAX - 1] = {};
    uint64_t first() const { return n ? len[0] : 0; }
};

// MDRP_CHUNKS: the positive entries of the comma-separated `spec`, at most NC_MAX - 1.  False where it is not set (null):
// default_lead chooses.  Set and empty: no leading chunk, the first super-chunk is one chunk.
inline bool parse_chunks(const char *spec_or_null, Lead &lead) {
    lead = Lead{};
    if (!spec_or_null) return false;
    const std::string spec = spec_or_null;
    size_t pos = 0;
    while (pos < spec.size() && lead.n < NC_MAX - 1) {
        const size_t q = spec.find(',', pos);
        const long v = atol(spec.substr(pos, q == std::string::npos ? std::string::npos : q - pos).c_str());
        if (v > 0) lead.len[lead.n++] = (uint64_t)v;
        if (q == std::string::npos) break;
        pos = q + 1;
    }
    return true;
}

// A SUPER-CHUNK is a range of iterations that shares one LO + walk pass and one host read-back; it is swept in one or
// more CHUNKS (solve / count / bound / score / scan launch trains).  Inside the certain range nothing can stop, so the
// first super-chunk is split into a short chunk (128 iterations) that establishes the records and the rest, whose
// hypotheses are retired against those records by k_count (MFMA) and k_bound (fp32) unless they might break one.
// Beyond the certain range a super-chunk is one chunk sized by the largest remaining dynamic_max_iter.
// The first chunk has no records of a chunk before it to retire anything against (what the 3-point estimators retire inside it, by the prefix
// records of a few hypotheses scored first, is first_pick's business below): keep it short.  Every later chunk goes
// through k_count / k_bound against the records of the chunks before it.  Measured on the benchmark shape: "128" 84.5 k pairs/s, "64" 82 k,
// "256" 82.5 k, "512" 82 k, "256,768" 79 k (every chunk costs ~10 launches and a solver hand-over).  The 7-point estimator gets a second leading
// chunk: at 50 % outliers one sample in 128 is outlier-free, so the records after 128 iterations are often those of a poor model and the rest of
// the run would be counted and bounded against a bar that retires little (round 6: k_bound 5.7 ms of a 16.4 ms step; with "128,1024" the bar
// the last 8848 iterations meet is that of 1152: 62.3 -> 87.3 k pairs/s; "128,512" 86.6 k, "256,1024" 87.6 k, "128,3300,3300" 78.3 k)
//
// Round 6, with the two-phase count: at 50 % outliers the step is flat in the first chunk's length from 128 to 512 iterations (calibrated P3P
// 8.45-8.49 / 8.44-8.55 / 8.40-8.41 / 8.51-8.66 ms at 128 / 256 / 384 / 512; shared focal 8.05 -> 7.99 at 256 or 384) — what a longer first
// chunk costs in exact scoring it returns as a tighter bar — but NOT at other outlier ratios: one 3-point sample in 64 is outlier-free at
// 75 % outliers, one in 300 at 85 %, and a pair whose first chunk holds none sends the whole rest of its run through the fp32 bound and the
// exact sweep: 75 % outliers 124 k pairs/s with 128, 142 k with 256, 147 k with 384; 85 %: 78 k / 93 k / 104 k (136 k with 1024).  The
// outlier-free shape pays for it the other way round (every hypothesis of the first chunk is a good one and is scored in full: 72.3 k with
// 128, 71.1 k with 256, 69.5 k with 384).  Default: 256 for the 3-point estimators where the run is long enough to pay for it (a sixteenth of
// the iterations that certainly run, between 128 and 256), up to 512 for the 5-point one by the same rule (solver-bound: flat), 128,1024 for the 7-point one
// (above), 128 for the 6-point one; MDRP_CHUNKS=384 or 128,1024 for data with fewer than one inlier in four.
constexpr uint64_t LEAD_5PT_MAX = 512;
// What estimate_device sizes a pass with before any pass has chosen its leading chunks: the longest default first chunk of the one estimator whose
// scratch depends on it (the 5-point solver's second Reduce5 region, PassScratch).
constexpr uint64_t LEAD_BUDGET = LEAD_5PT_MAX;
// `seen_wish`: the mean first_chunk_wish over the results of the handle's previous call with this 3-point estimator, or negative
inline Lead default_lead(int kind, uint64_t certain, double seen_wish) {
    const uint64_t sixteenth = std::max<uint64_t>(128, certain / 16 / 64 * 64);
    Lead lead;
    lead.n = 1;
    if (kind == MDRP_FUNDAMENTAL_7PT) { lead.n = 2; lead.len[0] = 128; lead.len[1] = 1024; }
    else if (kind == MDRP_SHARED_6PT) lead.len[0] = 128;
    else if (kind == MDRP_RELPOSE_5PT) lead.len[0] = std::min<uint64_t>(LEAD_5PT_MAX, sixteenth);
    else {
        lead.len[0] = std::min<uint64_t>(256, sixteenth);
        // ... and where the handle's previous call with this estimator (kind 0..2 here) has results to go by: the mean over its pairs of what each
        // would have liked (first_chunk_wish, mdrp_kernels.h: 6 / r^3 iterations for the pair's inlier ratio r, between 256 and 1024; 128 for nearly
        // outlier-free pairs) — the lengths the sweeps above found best at 0, 50, 75 and 85 % outliers, and for a batch that mixes them (20 / 50 / 70 /
        // 85 % by pair: 93.7 k pairs/s at 128, 101 k at 256, 105 k at 384-512, 104 k at 1024).  A long run only (the first chunk stays under an
        // eighth of it).
        if (seen_wish >= 0.0 && certain >= 8192) lead.len[0] = (uint64_t)std::min(1024.0, std::max(128.0, std::ceil(seen_wish / 64.0) * 64.0));
    }
    return lead;
}

// the chunks of the super-chunk that starts at iteration it0: their lengths, their offsets in the super-chunk and its length
struct Layout {
    int n_chunks = 1;
    uint64_t lens[NC_MAX] = {};
    int offs[NC_MAX] = {};
    uint64_t super_len = 0;
};
// `max_needed`: the largest dynamic_max_iter the pairs still iterating have left (beyond the certain range)
inline Layout super_chunk_layout(uint64_t it0, uint64_t certain, int chunk_cap, const Lead &lead, uint64_t max_needed, uint64_t max_iterations) {
    Layout l;
    if (it0 < certain) {
        const uint64_t span = std::min<uint64_t>(certain - it0, (uint64_t)chunk_cap);
        uint64_t used = 0;
        l.n_chunks = 0;
        if (it0 == 0)
            for (int i = 0; i < lead.n; ++i) { // a leading chunk only while at least as much again remains behind it
                if (used + 2 * lead.len[i] > span) break;
                l.lens[l.n_chunks++] = lead.len[i]; used += lead.len[i];
            }
        l.lens[l.n_chunks++] = span - used;
    } else {
        l.lens[0] = std::min<uint64_t>(std::min<uint64_t>(std::max<uint64_t>(max_needed, 256), max_iterations - it0), (uint64_t)chunk_cap);
    }
    for (int c = 0; c < l.n_chunks; ++c) l.super_len += l.lens[c];
    for (int c = 1; c < l.n_chunks; ++c) l.offs[c] = l.offs[c - 1] + (int)l.lens[c - 1];
    return l;
}

// one sample table per distinct correspondence count, numbered in order of first appearance
inline void group_tables(const int32_t *n_per_pair, int batch, std::vector<int32_t> &table_of, std::vector<int32_t> &tab_n) {
    table_of.assign(batch, 0); tab_n.clear();
    std::map<int32_t, int32_t> ids;
    for (int i = 0; i < batch; ++i) {
        auto it = ids.find(n_per_pair[i]);
        if (it == ids.end()) { it = ids.emplace(n_per_pair[i], (int32_t)tab_n.size()).first; tab_n.push_back(n_per_pair[i]); }
        table_of[i] = it->second;
    }
}

// pairs of one pass: what half of the free memory holds (at most 96 GiB of it) at `per_pair` bytes of scratch each
inline int pairs_per_pass(size_t free_bytes, size_t per_pair, int batch) {
    const size_t budget = std::min<size_t>((size_t)(0.5 * (double)free_bytes), (size_t)96 << 30);
    const int per_pass = (int)std::max<size_t>(1, std::min<size_t>((size_t)batch, budget / per_pair));
    return std::min(per_pass, 65535); // k_solve / k_probe put the pair index on grid.y
}

// Lanes per LO problem: one wavefront when there are many short problems; four when the batch is small or the pairs are large (N = 5000:
// a one-wavefront problem is 4 ms long and the launch ends with its stragglers — 45.6 against 43.9 ms per 1024 varying-focal pairs).
// Chosen from the CALL's batch, not a pass's: the lane count fixes the LM's summation tree, and how a call is cut into passes depends on the
// memory that happens to be free — a pair must get the same record whatever pass it falls into.
inline int lo_lanes(int batch_call, int n_max) { return (batch_call >= 128 && n_max < 4096) ? 64 : 256; }
inline int final_lanes(int batch_call) { return batch_call >= 4096 ? 64 : 256; }

// The first chunk's prefix retirement (k_first_pick / k_first_score / k_first_filter, mdrp_kernels.h): hypotheses picked per pair, 0 = the stage is
// off and the whole chunk goes to the exact sweep as before.  On for the 3-point estimators in calls that do not score by wavefront (`wave_max_pairs`:
// SCORE_WAVE_MAX_PAIRS); the 5-, 6- and 7-point estimators keep their front.  `knob`: MDRP_FIRST_PICK, or negative where it is not set.
constexpr int FIRST_PICK = 48, FIRST_PICK_LIMIT = 64;
inline int first_pick(int kind, int batch_call, int wave_max_pairs, int knob) {
    if (kind > MDRP_VARYING_FOCAL || batch_call <= wave_max_pairs) return 0;
    return knob < 0 ? FIRST_PICK : std::min(knob, FIRST_PICK_LIMIT);
}

// The solver beside a first chunk's sweeps.  A solver wavefront shares nothing with its neighbours, so one-wavefront workgroups refill a freed slot at
// once and the kernel alone is a quarter shorter (mdrp_kernels.h, k_solve) — but the 3-point calibrated solvers hold 152 VGPRs, three wavefronts per
// SIMD, and a 128-VGPR sweep wavefront finds no room beside three of them.  What a launch can still decide is its dynamic LDS: workgroups that each
// reserve `bytes` of it (never touched) fit floor(lds_per_cu / bytes) to a CU.  The rule: the bytes per solver workgroup at which exactly 4 R of them
// fit (R per SIMD) while `keep_free` bytes of the CU's LDS stay out of their reach — or 0, "uncapped", where R is not positive or no such size
// exists.  Both conditions at once need  lds / (4 R + 1) < bytes <= (lds - keep_free) / (4 R),  that is keep_free < lds / (4 R + 1): a solver capped
// through LDS takes at least 4 R / (4 R + 1) of it.  On 160 KiB and R = 2 that leaves 17.7 KiB, less than any sweep workgroup of the front needs
// (32 - 39 KiB), so with the sweeps' LDS kept free the rule answers "uncapped" there and the long solver keeps its four-wavefront workgroups;
// MDRP_SOLVE_RESIDENT = R asks for the cap without keeping anything free (DESIGN.md 4 has what that measures).
constexpr size_t LDS_GRANULE = 2560; // sizes are rounded down to a multiple of both LDS allocation granularities (512 B; 1280 B on parts with 160 KiB)
inline size_t solver_reservation(size_t lds_per_cu, int resident_per_simd, size_t keep_free) {
    if (resident_per_simd <= 0 || keep_free >= lds_per_cu) return 0;
    const size_t wgs = 4 * (size_t)resident_per_simd;
    const size_t bytes = (lds_per_cu - keep_free) / wgs / LDS_GRANULE * LDS_GRANULE;
    if (bytes == 0 || (wgs + 1) * bytes <= lds_per_cu) return 0; // one more would fit: no cap at this size
    return bytes;
}
constexpr int SOLVE_RESIDENT = 2; // R of the 3-point calibrated solvers where the first chunk's prefix retirement is on

// What the solver of a run's SECOND chunk (the long one, on the solver stream) waits for.  It reads the records and pair states k_prep (and a
// prior's kernel) leave and its own sample table, and writes the models, tags and model counts of its own chunk parity (the 5-point solver: its own
// Reduce5 region): nothing the first chunk's solver touches.  So it starts behind k_prep, beside the first chunk's solver (which is issued first and
// takes the head of the dispatch order), where
//  - the pass has device-resident inputs (the sliced host-buffer front issues that solver slice by slice itself),
//  - the second chunk's sample table was drawn ahead on the LO stream (otherwise the sampler advances the tables in chunk order on the solver's stream),
//  - the estimator is not the 6-point one: its solver takes 11.5 KB of scratch per lane, and two of its dispatches on two queues at once need two
//    whole-device scratch areas (Pass::first_chunk_of, mdrp_capi.hip).
// Otherwise, and with MDRP_SOLVE_BEHIND_PREP=0 (`knob`; negative: not set), it waits for the first chunk's solver as it always did.  The third and later
// chunks wait for the scan of the chunk whose lists they reuse whatever this says.
enum class SolveAfter { prep, first_solver };
inline SolveAfter second_solver_after(int kind, bool presampled, bool host_buffers, int n_chunks, int knob) {
    if (knob == 0 || host_buffers || !presampled || n_chunks < 2 || kind == MDRP_SHARED_6PT) return SolveAfter::first_solver;
    return SolveAfter::prep;
}

// Bounded waits of the fused tail (k_gate, k_final), microseconds: far beyond anything a healthy run needs (the LO queue of 1024 pairs is empty
// after ~1 ms), scaled with the problem size (one LO problem is ~0.4 ms at N = 2000 and grows linearly with N: 4 ms at 5000 on one wavefront) and
// capped at 200 ms / 100 ms: under persistently serialised dispatch (rocprofv3 --pmc, AMD_SERIALIZE_KERNEL, a debugger) every re-try of the
// fused tail pays these in full (3.3 s at N = 70001 before the cap)
inline long long fuse_n_scale(int n_max) { return std::max(1, (n_max + 1999) / 2000); }
inline int fuse_gate_us(int batch, int n_max) { return (int)std::min<long long>((50000 + 40ll * batch) * fuse_n_scale(n_max), 200000); }
inline int fuse_wait_us(int batch, int n_max) { return (int)std::min<long long>((20000 + 4ll * batch) * fuse_n_scale(n_max), 100000); }

} // namespace sched
} // namespace mdrp
