"""Yardstick of the bookkeeping train (k_scan, k_lo_plan, walk_pair, the budget checkpoints): the loop of orc_ransac
(oracle/orc_ransac.c) and prior_ref.ransac_from_prior in plain Python over TABLES instead of solvers.  A helper, not a test.

A pair's table gives, for iteration i and slot k, what the reference would have computed there: the model's inlier count and MSAC score (a negative
count: no model in this slot; -3 in slot 0: the NaN model, which scores (0, n * sq_thr)), an id that stands for the model, and the count, score and
id of that model's LO refinement.  `loop` walks it exactly as the reference walks its solver's output: both records of the minimal models, best_ind,
per-model adoption, refinements, inlier_ratio, the dynamic bound and the three-line stop test.  tests/test_replay_host.py pins it to pyorc's
orc_ransac on real pairs, with the tables filled from the oracle's own solvers, scorers and LM."""
import math
import types

import numpy as np

import prior_ref as pr

U64 = 2 ** 64
_DYN = {}  # dyn_max_iter by (ratio, options)
DBL_MAX = pr.DBL_MAX
STATE_FIELDS = ("n", "active", "sq_thr", "best_min_cnt", "best_min_score", "dyn_max_iter", "iterations", "refinements", "num_inliers", "inlier_ratio",
                "model_score", "best")


def options(max_iterations, min_iterations, dyn_mult=3.0, success_prob=0.9999, sample_sz=3):
    """the four stopping fields of RansacOptions and the sample size (the exponent of the inlier ratio in the dynamic bound)"""
    return types.SimpleNamespace(max_iterations=int(max_iterations), min_iterations=int(min_iterations), dyn_num_trials_mult=float(dyn_mult),
                                 success_prob=float(success_prob), sample_sz=int(sample_sz))


def log_prob_missing(opt):
    """log(1 - success_prob) as the C library computes it: -inf at success_prob = 1, NaN above"""
    x = 1.0 - opt.success_prob
    return np.float64(-math.inf if x == 0.0 else (math.nan if x < 0.0 else math.log(x)))


def bound_before_ceil(ratio, opt):
    """the dynamic bound as a real number, before ceil and the conversion to uint64_t; None on the two branches that do not compute one"""
    if ratio >= 0.9999 or ratio <= 0.0001:
        return None
    r = float(ratio)
    p = r * r * r if opt.sample_sz == 3 else math.pow(r, float(opt.sample_sz))
    with np.errstate(all="ignore"):
        return float(log_prob_missing(opt) / np.float64(math.log(1.0 - p)) * np.float64(opt.dyn_num_trials_mult))


def dyn_max_iter(ratio, opt):
    """ransac<>'s dynamic iteration bound: prior_ref's for sample size 3 (x * x * x), libm pow for 5 and 7"""
    if opt.sample_sz == 3:
        return pr.dyn_max_iter(ratio, opt, log_prob_missing(opt))
    if ratio >= 0.9999:
        return opt.min_iterations
    if ratio <= 0.0001:
        return opt.max_iterations
    v = bound_before_ceil(ratio, opt)
    return pr.f64_to_u64_x86(float(math.ceil(v)) if math.isfinite(v) else v)


def new_state(n, sq_thr, active=1, best_min_cnt=0, best_min_score=DBL_MAX, dyn_max_iter=0, iterations=0, refinements=0, num_inliers=0, inlier_ratio=0.0,
              model_score=DBL_MAX, best=0.0):
    return dict(n=int(n), active=int(active), sq_thr=float(sq_thr), best_min_cnt=int(best_min_cnt), best_min_score=float(best_min_score),
                dyn_max_iter=int(dyn_max_iter), iterations=int(iterations), refinements=int(refinements), num_inliers=int(num_inliers),
                inlier_ratio=float(inlier_ratio), model_score=float(model_score), best=float(best))


class Table:
    """one pair's slots from absolute iteration `start` on: cnt, score, ids, lo_score, lo_cnt, lo_ids, each [iterations][mps]"""

    def __init__(self, start, cnt, score, ids, lo_score, lo_cnt, lo_ids):
        self.start = int(start)
        self.cnt, self.score, self.ids = np.asarray(cnt, np.int32), np.asarray(score, np.float64), np.asarray(ids, np.float64)
        self.lo_score, self.lo_cnt, self.lo_ids = np.asarray(lo_score, np.float64), np.asarray(lo_cnt, np.int32), np.asarray(lo_ids, np.float64)
        self.len, self.mps = self.cnt.shape
        self._lists = None
        self._lim = None

    def lists(self):
        if self._lists is None:
            self._lists = tuple(a.tolist() for a in (self.cnt, self.score, self.ids, self.lo_score, self.lo_cnt, self.lo_ids))
        return self._lists

    def limits(self, nan_score):
        """per iteration, the largest count and the smallest score any of its models has (the -3 slot converted): an iteration whose largest count
        does not exceed the record and whose smallest score is not below it cannot change anything — `loop` may skip it unread (fast=True)"""
        if self._lim is None or self._lim[0] != nan_score:
            c, s = self.cnt.astype(np.int64), self.score.copy()
            nanm = c[:, 0] == -3
            c[nanm, 0], s[nanm, 0] = 0, nan_score
            s[c < 0] = np.inf
            s[np.isnan(s)] = np.inf
            self._lim = (nan_score, np.where(c >= 0, c, -1).max(axis=1).tolist(), s.min(axis=1).tolist())
        return self._lim[1], self._lim[2]


def loop(tab, state, opt, upto, stop=True, max_iterations=None, fast=True):
    """The reference's loop from state['iterations'] (its next iteration) until the stop test fires or iteration `upto` is reached.
    stop=False: no stop test at all — what the scans see, which run over a super-chunk before anyone knows where the pair stops.
    max_iterations=K: the run with that maximum (DESIGN.md 12's definition of the result at budget K).
    Returns (state, triggers, dyn_from_max): the new state (active = 0 once stopped), the iterations that broke a record as dicts(iter: absolute,
    k_ref, k_min, cnt_min, score_min, cnt_ref), and whether the dynamic bound in the state was last copied from max_iterations."""
    st = dict(state)
    trig = []
    dyn_from_max = False
    if not st["active"]:
        return st, trig, dyn_from_max
    cnt, score, ids, lo_score, lo_cnt, lo_ids = tab.lists()
    maxit = opt.max_iterations if max_iterations is None else int(max_iterations)
    o = opt if max_iterations is None else options(maxit, opt.min_iterations, opt.dyn_num_trials_mult, opt.success_prob, opt.sample_sz)
    n, nan_score = st["n"], float(np.float64(st["n"]) * np.float64(st["sq_thr"]))
    lim_c, lim_s = tab.limits(nan_score) if fast else (None, None)
    best_min_cnt, best_min_score = st["best_min_cnt"], st["best_min_score"]
    it = st["iterations"]
    while True:
        if stop and it >= maxit:  # the loop head (max_iterations = 0: no sample is drawn)
            st["active"] = 0
            break
        if it >= upto:
            break
        row = it - tab.start
        best_ind = -1
        if not fast or lim_c[row] > best_min_cnt or lim_s[row] < best_min_score:
            k_min, cnt_min, score_min = -1, 0, 0.0
            for k in range(tab.mps):
                c, s = cnt[row][k], score[row][k]
                if k == 0 and c == -3:
                    c, s = 0, nan_score
                elif c < 0:
                    continue
                more, better = c > best_min_cnt, s < best_min_score
                if more or better:
                    if more:
                        best_min_cnt = c
                    if better:
                        best_min_score = s
                        k_min, cnt_min, score_min = k, c, s
                    best_ind = k
                    if s < st["model_score"]:
                        st["model_score"], st["best"], st["num_inliers"] = s, ids[row][k], c
        if best_ind >= 0:
            c0 = cnt[row][best_ind]
            trig.append(dict(iter=it, k_ref=best_ind, k_min=k_min, cnt_min=cnt_min, score_min=score_min, cnt_ref=0 if c0 == -3 else c0))
        if best_ind >= 0 and stop:  # (the scans only list the record breakers: the LO and the bookkeeping behind it belong to the walk)
            st["refinements"] += 1
            s, c = lo_score[row][best_ind], lo_cnt[row][best_ind]
            if s < st["model_score"]:
                st["model_score"], st["num_inliers"], st["best"] = s, c, lo_ids[row][best_ind]
            st["inlier_ratio"] = st["num_inliers"] / n
            key = (st["inlier_ratio"], o.max_iterations, o.min_iterations, o.dyn_num_trials_mult, o.success_prob, o.sample_sz)
            if key not in _DYN:
                _DYN[key] = dyn_max_iter(st["inlier_ratio"], o)
            st["dyn_max_iter"] = _DYN[key]
            dyn_from_max = st["inlier_ratio"] <= 0.0001 and not st["inlier_ratio"] >= 0.9999
        it = (it + 1) % U64
        if not stop:
            continue
        if it >= maxit:
            st["active"] = 0
            break
        if it <= o.min_iterations:
            continue
        if it > st["dyn_max_iter"]:
            st["active"] = 0
            break
    st["iterations"] = it
    st["best_min_cnt"], st["best_min_score"] = best_min_cnt, best_min_score
    return st, trig, dyn_from_max


def need_of(st, opt):
    """iterations an active pair still certainly needs: first value s > iterations at which the stop test fires, minus iterations (no wrap-around:
    a bound of 2^64 - 1 is never exceeded, so only max_iterations ends such a run)"""
    it = st["iterations"]
    s = max(it + 1, min(opt.max_iterations, max(opt.min_iterations + 1, st["dyn_max_iter"] + 1)))
    return s - it


def super_chunk(tab, state, opt, chunk_start, chunk_lens, budgets=()):
    """What one super-chunk [chunk_start, chunk_start + sum(chunk_lens)) leaves behind, as the phase-split form must report it:
    dict(state: the loop's state at the end, with the records of the minimal models as the scans leave them (a scan runs to the end of the
    super-chunk even where the pair stops inside it); chunk_triggers: per chunk, the record breakers the scan of that chunk emits; records: (count,
    score) behind each chunk; executed: the triggers the loop executed; checkpoints: {K: (state, dyn_from_max)} for the budgets in (chunk_start, end],
    and every later one when the pair stopped)"""
    c1 = chunk_start + sum(chunk_lens)
    out = dict(state=dict(state), chunk_triggers=[[] for _ in chunk_lens], records=[(state["best_min_cnt"], state["best_min_score"])] * len(chunk_lens),
               executed=[], checkpoints={})
    if not state["active"]:
        return out
    assert state["iterations"] == chunk_start
    sc = dict(state)
    for c, ln in enumerate(chunk_lens):
        sc, tr, _ = loop(tab, sc, opt, sc["iterations"] + ln, stop=False)
        out["chunk_triggers"][c] = tr
        out["records"][c] = (sc["best_min_cnt"], sc["best_min_score"])
    st, ex, _ = loop(tab, state, opt, c1)
    out["executed"] = ex
    for K in budgets:
        if K > chunk_start and (K <= c1 or not st["active"]):
            ck, _, from_max = loop(tab, state, opt, c1, max_iterations=K)
            assert not ck["active"], K
            out["checkpoints"][int(K)] = (ck, from_max)
    st["best_min_cnt"], st["best_min_score"] = sc["best_min_cnt"], sc["best_min_score"]
    out["state"] = st
    return out
