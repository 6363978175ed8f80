"""Planted inputs of the bookkeeping train's tests (tests/test_gpu_replay.py, tests/test_replay_host.py).  A helper, not a test.  Seeded and
deterministic; counts and scores are arbitrary numbers, there is no geometry.

Every planted start state keeps the invariant the estimator guarantees: model_score <= best_min_score, with num_inliers and inlier_ratio consistent
(inlier_ratio = num_inliers / n).  walk_pair adopts a minimal model through the trigger's k_min alone; that equals the reference's per-model adoption
ONLY under this invariant (a model that has more inliers without a better score than the record then cannot score below model_score), so a start
state that broke it would test something the estimator never does.

Counts that can become num_inliers are kept away from the places where the dynamic bound, before ceil, lies within 1e-9 (relative) of an integer: the
device's log and pow need not be bit-equal to libm's.  A drawn count that fails the condition is redrawn (REDRAWS counts them against DRAWS);
tests/test_replay_host.py asserts the condition on the finished tables.  Counts are 0 or at least floor_of(n, sample size): a smaller ratio above
0.0001 gives bounds so large that no count passes."""
import functools
import math

import numpy as np

import replay_ref as rr

DBL_MAX = rr.DBL_MAX
SQ_THR = 2.5e-7
DRAWS, REDRAWS = [0], [0]
PATTERNS = ("staircase", "more_only", "better_only", "ties", "sequences", "positions", "special", "sparse")
STARTS = ("fresh", "initial", "carried", "inactive", "empty", "dyn63", "dyn_m2", "dyn_m1")
LO_KINDS = ("below", "equal", "above", "nan", "max")


_SAFE = {}


def floor_of(n, sample_sz):
    """the smallest planted count above 0: ratio^sample_sz >= 3e-4 keeps the bound below ~1e5 at the default options, where one count in 10^4 fails
    the input condition"""
    return max(1, math.ceil(n * 3e-4 ** (1.0 / sample_sz)))


def safe_count(c, n, opt):
    """the input condition: the bound before ceil at least 1e-9 relative away from every integer (or no finite bound at all)"""
    key = (c, n, opt.dyn_num_trials_mult, opt.success_prob, opt.sample_sz)
    ok = _SAFE.get(key)
    if ok is None:
        v = rr.bound_before_ceil(c / n, opt)
        ok = _SAFE[key] = v is None or not math.isfinite(v) or abs(v - round(v)) >= 1e-9 * abs(v)
    return ok


class Gen:
    """fills one pair's table row by row, keeping the running records and model_score the loop will have, so that a slot can be planted as a tie, a
    record breaker of one kind or neither"""

    def __init__(self, seed, pair, mps, n, opt, state, start, rows):
        rng = self.rng = np.random.default_rng(seed)
        self.mps, self.n, self.opt, self.start, self.rows = mps, n, opt, start, rows
        self.floor = floor_of(n, opt.sample_sz)
        self.rc, self.rs, self.ms = state["best_min_cnt"], state["best_min_score"], state["model_score"]
        self.nan_score = float(np.float64(n) * np.float64(state["sq_thr"]))
        self.cnt = np.full((rows, mps), -1, np.int32)
        self.score = rng.uniform(1e-12, 1e-9, (rows, mps))  # stale scores of empty slots: below every record
        base = (pair * (1 << 22) + np.arange(rows * mps, dtype=np.float64).reshape(rows, mps)) * 2.0
        self.ids, self.lo_ids = base + 1.0, base + 2.0
        # LO results nobody may read: adopting one would end the run at once (ratio 1)
        self.lo_score, self.lo_cnt = np.full((rows, mps), 1e-30), np.full((rows, mps), n, np.int32)
        self.u = rng.random((rows, mps, 2)).tolist()      # two uniform numbers per slot, three per row
        self.ur = rng.random((rows, 3)).tolist()
        self.dk = rng.integers(0, 6, (rows, mps)).tolist()

    def count(self, lo, hi, u):
        """a count in [lo, hi] that is 0 or >= floor and meets the input condition"""
        DRAWS[0] += 1
        c = lo + int(u * (hi - lo + 1))
        if 0 < c < self.floor:
            c = 0 if lo <= 0 else min(max(self.floor, lo), hi)
        while not safe_count(c, self.n, self.opt):
            REDRAWS[0] += 1
            c += 1
        assert c <= self.n
        return c

    def pick(self, i):
        return int(self.ur[i][0] * self.mps)

    def row(self, i, kinds, lo="below", lo_cnt=None):
        """plant iteration i (table row): one kind per slot — e empty, r no record, d dull, t exact tie with both records, m more only, b better only,
        x both, N the NaN model (slot 0), q a NaN score with a dull count, Q a NaN score with more inliers.  Then the LO result of the slot the
        iteration refines, `lo` relative to model_score as it is when the LO result is looked at."""
        best_ind = -1
        for k, kind in enumerate(kinds):
            if kind == "e":
                continue
            if kind == "r":
                self.cnt[i, k], self.score[i, k] = -2, DBL_MAX
                continue
            u0, u1 = self.u[i][k]
            if kind == "N":
                assert k == 0
                self.cnt[i, k] = -3
                c, s = 0, self.nan_score
            else:
                if kind in "mxQ" and self.rc + 4 > self.n:  # (the counts have run out)
                    kind = {"m": "d", "x": "b", "Q": "q"}[kind]
                if kind in "mxQ":
                    c = self.count(self.rc + 1, max(self.rc + 1, self.floor) + 3, u0)
                elif kind == "t":
                    c = self.rc
                else:
                    c = self.count(0, self.rc, u0) if self.rc >= self.floor else 0
                if kind in "qQ":
                    s = math.nan
                elif kind == "t":
                    s = self.rs
                elif kind in "bx":
                    s = self.nan_score * (0.5 + 0.4 * u1) if self.rs >= DBL_MAX else self.rs * (1.0 - 1e-4 - 1.9e-3 * u1)
                else:
                    s = DBL_MAX if self.rs >= DBL_MAX else self.rs * (1.0 + 1e-6 + 0.5 * u1)
                self.cnt[i, k], self.score[i, k] = c, s
            more, better = c > self.rc, s < self.rs
            if more or better:
                if more:
                    self.rc = c
                if better:
                    self.rs = s
                best_ind = k
                if s < self.ms:
                    self.ms = s
        if best_ind < 0:
            return False
        u = 1e-3 + 0.2 * self.ur[i][1]
        s = dict(below=self.ms * (1.0 - u) if self.ms < DBL_MAX else self.nan_score * 0.4, equal=self.ms, above=self.ms * (1.0 + u) if self.ms < DBL_MAX / 2 else DBL_MAX,
                 nan=math.nan, max=DBL_MAX)[lo]
        self.lo_score[i, best_ind] = s
        self.lo_cnt[i, best_ind] = self.count(self.floor, self.n - 1, self.ur[i][2]) if lo_cnt is None else lo_cnt
        if s < self.ms:
            self.ms = s
        return True

    def dull(self, i):
        return ["eerddt"[j] for j in self.dk[i]]

    def table(self):
        return rr.Table(self.start, self.cnt, self.score, self.ids, self.lo_score, self.lo_cnt, self.lo_ids)


def start_state(kind, pair, n, opt, chunk_start, rng):
    best = -1.0 - pair
    nan_score = float(np.float64(n) * np.float64(SQ_THR))
    if kind == "empty":
        return rr.new_state(0, SQ_THR, active=0, dyn_max_iter=opt.max_iterations, best=best)
    if kind == "inactive":  # a pair that stopped earlier
        c = max(1, n // 3)
        return rr.new_state(n, SQ_THR, active=0, best_min_cnt=c, best_min_score=nan_score * 0.5, dyn_max_iter=7, iterations=8, refinements=3, num_inliers=c,
                            inlier_ratio=c / n, model_score=nan_score * 0.4, best=best)
    if kind == "initial" and chunk_start == 0:  # after score_initial_model: records (0, n * sq_thr), one refinement
        return rr.new_state(n, SQ_THR, best_min_score=nan_score, dyn_max_iter=opt.max_iterations, refinements=1, model_score=nan_score, best=best)
    if kind == "carried" or chunk_start > 0:  # left by an earlier super-chunk or a prior: model_score < best_min_score
        c = floor_of(n, opt.sample_sz) + int(rng.integers(0, max(1, n // 50)))
        while not safe_count(c, n, opt):
            c += 1
        dyn = rr.dyn_max_iter(c / n, opt)
        if chunk_start > opt.min_iterations and chunk_start > dyn:  # (such a pair would have stopped: it starts with the bound of a run that found nothing)
            c, dyn = 0, opt.max_iterations
        return rr.new_state(n, SQ_THR, best_min_cnt=c + 2 if c else 0, best_min_score=nan_score * 0.7, dyn_max_iter=dyn, iterations=chunk_start, refinements=4,
                            num_inliers=c, inlier_ratio=c / n, model_score=nan_score * 0.6, best=best)
    st = rr.new_state(n, SQ_THR, dyn_max_iter=opt.max_iterations, best=best)  # fresh
    if kind in ("dyn63", "dyn_m2", "dyn_m1"):  # a bound the conversion of a NaN or a negative double leaves: never exceeded
        st["dyn_max_iter"] = {"dyn63": 1 << 63, "dyn_m2": 2 ** 64 - 2, "dyn_m1": 2 ** 64 - 1}[kind]
    return st


def positions_of(chunk_lens):
    """iterations that must break a record: the first and last of every chunk, both sides of the 64- and 256-iteration step boundaries, lanes 0 and
    63, and all four iterations of one lane's group of four (two of them alone in another group)"""
    pos, off = set(), 0
    for ln in chunk_lens:
        for q in (0, ln - 1, 63, 64, 127, 128, 20, 21, 22, 23, 41, 43, 252, 255, 256, 257, 1023, 1024):
            if 0 <= q < ln:
                pos.add(off + q)
        off += ln
    return pos


def fill(g, pattern, plant_lens, lo_cycle):
    """one pattern over the whole table; plant_lens: the chunk schedules whose edges the `positions` pattern plants; lo_cycle: offset into LO_KINDS"""
    mps, rows = g.mps, g.rows
    planted = set().union(*[positions_of(lens) for lens in plant_lens]) if pattern == "positions" else set()
    sparse_next = 0
    nlo = 0
    for i in range(rows):
        lo = LO_KINDS[(lo_cycle + nlo) % len(LO_KINDS)]
        kinds = g.dull(i)
        at, u = g.pick(i), g.ur[i][1]
        if pattern == "staircase":  # every iteration breaks a record
            kinds[at] = "mbx"[i % 3]
        elif pattern == "more_only":
            if i % 5 != 3:
                kinds[at] = "m"
        elif pattern == "better_only":
            if i % 7 != 2:
                kinds[at] = "b"
        elif pattern == "ties":  # ties in every slot; a breaker every 50 iterations moves the records the neighbours then tie with
            kinds = ["t"] * mps
            if i % 50 == 10:
                kinds[mps - 1] = "x"
        elif pattern == "sequences":
            if i % 3 == 0:  # better, more-not-better, neither, better again | ... and the variant that ends on "more": k_ref != k_min
                a0 = at % (mps - 3)
                kinds[a0:a0 + 4] = ["b", "m", "d", "b"] if i % 6 == 0 else ["b", "d", "m", "e"]
        elif pattern == "positions":
            if i in planted:
                kinds[at] = "mbx"[int(u * 3)]
        elif pattern == "special":
            r = i % 8
            if r == 0:
                kinds[0] = "N"  # against no record (a fresh run's first iteration) or a record it cannot beat
            elif r == 1:
                kinds = ["e"] * mps
            elif r == 2:
                kinds = ["r"] * mps
            elif r == 3:
                kinds[at] = "Q"
            elif r == 4:
                kinds[at] = "q"
            elif r == 5:
                kinds[at] = "b"
        elif pattern == "sparse":  # records fall geometrically
            if i >= sparse_next:
                kinds[at] = "mbx"[int(u * 3)]
                sparse_next = i + 1 + int(-math.log(1.0 - g.ur[i][2]) * (2.0 + 0.5 * i))
        nlo += g.row(i, kinds, lo)


def make_case(name, mps, sample_sz, opt, chunk_start, supers, batch, seed, budgets=None, patterns=PATTERNS, starts=STARTS, n=5000, distinct=None,
              plant_lens=None):
    """dict(name, mps, opt, chunk_start, supers: the chunk lengths of each super-chunk of the chain, budgets, states, tables, patterns, starts).
    distinct: only that many tables are generated; pair p uses table p % distinct from its own start state (any table is a valid input of any state)"""
    rows = sum(sum(s) for s in supers)
    plant_lens = plant_lens or [[ln for s in supers for ln in s]]
    distinct = distinct or batch
    states, tables, pats, sts = [], [], [], []
    for p in range(batch):
        pat, skind = patterns[p % len(patterns)], starts[(p // len(patterns) + p) % len(starts)]
        st = start_state(skind, p, n, opt, chunk_start, np.random.default_rng([seed, p, 1]))
        if p < distinct:
            g = Gen([seed, p, 2], p, mps, n, opt, st if st["n"] else start_state("fresh", p, n, opt, 0, None), chunk_start, rows)
            fill(g, pat, plant_lens, p)
            tables.append(g.table())
        else:
            tables.append(tables[p % distinct])
        states.append(st)
        pats.append(pats[p % distinct] if p >= distinct else pat)
        sts.append(skind)
    return dict(name=name, mps=mps, opt=opt, chunk_start=chunk_start, supers=[list(s) for s in supers], budgets=budgets, states=states, tables=tables,
                patterns=pats, starts=sts)


def _opt(sample_sz, max_it=10 ** 6, min_it=10 ** 6, mult=3.0, prob=0.9999):
    return rr.options(max_it, min_it, mult, prob, sample_sz)


SAMPLE_OF = {4: 3, 12: 5, 16: 7}
EDGE_LENS = (1, 63, 64, 65, 255, 256, 257)


def head_of(case, rows, name):
    """the case on the first `rows` iterations of its tables, as one chunk"""
    tabs = {}
    for t in case["tables"]:
        if id(t) not in tabs:
            tabs[id(t)] = rr.Table(t.start, t.cnt[:rows], t.score[:rows], t.ids[:rows], t.lo_score[:rows], t.lo_cnt[:rows], t.lo_ids[:rows])
    return dict(case, name=name, supers=[[rows]], tables=[tabs[id(t)] for t in case["tables"]])


@functools.lru_cache(maxsize=None)
def _edge_base(mps):
    return make_case(f"edge{mps}", mps, SAMPLE_OF[mps], _opt(SAMPLE_OF[mps]), 0, [[max(EDGE_LENS)]], 65, 100 + mps, plant_lens=[[ln] for ln in EDGE_LENS])


@functools.lru_cache(maxsize=None)
def edge_case(mps, ln):
    """one chunk of an edge length, nothing stops (min_iterations beyond the end): 65 pairs, every pattern and start state"""
    return head_of(_edge_base(mps), ln, f"edge{mps}_{ln}")


LONG_LENS = (1024, 1025, 1279)


@functools.lru_cache(maxsize=None)
def long_case(mps, ln):
    """chunks of 1024 iterations and more (four iterations per lane where mps = 4, ragged last steps), in batches of 1, 64 and 130 pairs; the largest
    table is 130 pairs x 1279 iterations x 16 slots.  The first pair's staircase fills the whole trigger list."""
    batch = {1024: 1, 1025: 64, 1279: 130 if mps == 16 else 8}[ln]
    return make_case(f"long{mps}_{ln}", mps, SAMPLE_OF[mps], _opt(SAMPLE_OF[mps]), 0, [[ln]], batch, 200 + ln + mps, distinct=min(batch, 8),
                     starts=("fresh",) if batch == 1 else STARTS)


MULTI = dict(a=[[64, 65, 191]], b=[[128, 1100]], chain=[[63, 65], [256], [1024, 100]], chain_b=[[1024, 484]], chain_c=[[1508]])


@functools.lru_cache(maxsize=None)
def multi_case(mps, which):
    """several chunks per super-chunk; `chain`: three super-chunks with stops on the way; `chain_b`, `chain_c`: the same tables in other splits"""
    stop = which.startswith("chain")
    if stop and which != "chain":
        return dict(multi_case(mps, "chain"), name=f"multi{mps}_{which}", supers=[list(x) for x in MULTI[which]])
    opt = _opt(SAMPLE_OF[mps], 1400, 300) if stop else _opt(SAMPLE_OF[mps])
    return make_case(f"multi{mps}_{which}", mps, SAMPLE_OF[mps], opt, 0, MULTI[which], 10, 300 + mps + len(which))


def _count_with_bound(n, opt, lo, hi, rng):
    """a safe count whose dynamic bound lies in [lo, hi]"""
    for c in rng.permutation(np.arange(floor_of(n, opt.sample_sz), n)).tolist():
        if lo <= rr.dyn_max_iter(c / n, opt) <= hi and safe_count(c, n, opt):
            return c
    raise AssertionError((lo, hi))


STOP_POSITIONS = ("between", "on_trigger", "after_trigger", "at_max", "nowhere")


@functools.lru_cache(maxsize=None)
def stop_case(sample_sz):
    """the first stop at each position of STOP_POSITIONS relative to the triggers, and the option edges; one pair each, one chunk of 200 iterations
    (k_scan for mps = 4; the walk does not depend on mps).  Returns (case, claims): claims[p] names what pair p is planted for."""
    n, rows, mps = 5000, 200, 4
    out = []
    rng = np.random.default_rng(900 + sample_sz)

    def pair(opt, plan, claim, start="fresh", lo_first="below", lo_cnt=None):
        """plan: {row: kind of the one breaker in it}; the first trigger's LO is adopted with lo_cnt inliers, every later one is `above`"""
        p = len(out)
        st = start_state(start, p, n, opt, 0, rng)
        g = Gen([901, sample_sz, p], p, mps, n, opt, st, 0, rows)
        first = True
        for i in range(rows):
            kinds = g.dull(i)
            if i in plan:
                kinds[i % mps] = plan[i]
            if g.row(i, kinds, lo_first if first else "above", lo_cnt if first else None):
                first = False
        out.append((opt, st, g.table(), claim))

    base = _opt(sample_sz, 10 ** 5, 20)
    c = _count_with_bound(n, base, 60, 120, rng)
    D = rr.dyn_max_iter(c / n, base)  # the run stops when iterations reaches D + 1, unless a later trigger moves the bound
    pair(base, {3: "x", D - 10: "m", D + 12: "m"}, "between", lo_cnt=c)
    pair(base, {3: "x", D + 1: "m"}, "on_trigger", lo_cnt=c)
    pair(base, {3: "x", D: "m"}, "after_trigger", lo_cnt=c)
    pair(base, {3: "x", D - 1: "m"}, "trigger_on_bound", lo_cnt=c)  # iterations == dyn_max_iter behind a trigger: not yet exceeded, one more iteration runs
    far = _opt(sample_sz, 150, 20)
    pair(far, {3: "x", 149: "m", 150: "b"}, "at_max", lo_cnt=_count_with_bound(n, far, 1000, 10 ** 5, rng))
    pair(_opt(sample_sz, 10 ** 5, 10 ** 4), {3: "x", 50: "b"}, "nowhere", lo_cnt=c)
    pair(_opt(sample_sz, 10 ** 5, 30, prob=1.0), {3: "x", 30: "m", 31: "m"}, "prob_one")           # bound +inf -> 0: stops at min_iterations + 1
    pair(_opt(sample_sz, 150, 30, prob=1.5), {3: "x", 100: "b"}, "prob_above_one")                 # NaN -> 2^63: runs to max_iterations
    pair(_opt(sample_sz, 10 ** 5, 30, mult=0.0), {3: "x", 40: "b"}, "mult_zero")                   # bound 0
    m1 = _opt(sample_sz, 180, 10, mult=-1.0, prob=0.5)
    cm = next(cc for cc in range(n // 2, n) if rr.dyn_max_iter(cc / n, m1) == 2 ** 64 - 1 and safe_count(cc, n, m1))
    pair(m1, {3: "x", 90: "b"}, "mult_minus_one", lo_cnt=cm)                                       # bound in (-2, -1] -> 2^64 - 1: runs to max_iterations
    pair(m1, {}, "dyn_m1_no_trigger", start="dyn_m1")
    pair(_opt(sample_sz, 180, 2 ** 64 - 1), {3: "x", 90: "b"}, "min_is_max_u64", lo_cnt=c)         # min_iterations + 1 must not wrap either
    pair(_opt(sample_sz, 0, 0), {0: "x", 5: "b"}, "max_zero")
    pair(_opt(sample_sz, 10 ** 5, 25), {3: "x"}, "ratio_high", lo_cnt=n)                           # >= 0.9999: the bound is min_iterations
    pair(_opt(sample_sz, 170, 25), {3: "x"}, "ratio_low", lo_cnt=0)                                # <= 0.0001: the bound is max_iterations
    return out


@functools.lru_cache(maxsize=None)
def stop_cases(sample_sz):
    """stop_case's pairs as one-pair cases (each has options of its own)"""
    assert tuple(c for _, _, _, c in stop_case(sample_sz)) == STOP_CLAIMS
    return [(dict(name=f"stop{sample_sz}_{claim}", mps=4, opt=opt, chunk_start=0, supers=[[200]], budgets=None, states=[st], tables=[tab], patterns=["stop"],
                  starts=["fresh"]), claim) for opt, st, tab, claim in stop_case(sample_sz)]


@functools.lru_cache(maxsize=None)
def budget_case(mps):
    """a chain of two super-chunks (96 | 64, then 140) with a budget list placed on the yardstick's own events per pair is not possible (one list per
    call), so the list is fixed and the PAIRS are planted around it: a trigger on a budget, on the iteration before it, the first trigger behind the
    first budget; a budget equal to the second call's chunk_start (160) and to the super-chunks' ends (160, 300); budgets behind a stop."""
    budgets = [10, 40, 41, 100, 160, 161, 250, 300]
    n, rows = 5000, 300
    opt = _opt(SAMPLE_OF[mps], 300, 50)
    rng = np.random.default_rng(700 + mps)
    c_stop = _count_with_bound(n, opt, 120, 200, rng)
    plans = [
        ({12: "x", 40: "m", 41: "b", 100: "x", 160: "b", 161: "m", 249: "x", 299: "b"}, None),   # triggers on budgets
        ({12: "x", 39: "m", 99: "b", 159: "x", 160: "m", 298: "b"}, None),                       # ... and on the iterations before them
        ({20: "x", 45: "b"}, None),                                                              # first trigger behind the first budget
        ({5: "x", 30: "b"}, c_stop),                                                             # stops between budgets 160 and 250 at the latest
        ({}, None),                                                                              # no trigger at all
    ]
    states, tables, pats, sts = [], [], [], []
    for p in range(66):
        plan, lo_cnt = plans[p % len(plans)]
        skind = ("fresh", "initial", "inactive", "empty")[(p // len(plans)) % 4] if p < 40 else "fresh"
        st = start_state(skind, p, n, opt, 0, rng)
        g = Gen([701, mps, p], p, mps, n, opt, st if st["n"] else start_state("fresh", p, n, opt, 0, None), 0, rows)
        first = True
        for i in range(rows):
            kinds = g.dull(i)
            if i in plan:
                kinds[(i + p) % mps] = plan[i]
            elif p >= 40 and rng.random() < 0.05:
                kinds[int(rng.integers(0, mps))] = "mbx"[int(rng.integers(0, 3))]
            if g.row(i, kinds, LO_KINDS[(p + i) % 5] if lo_cnt is None or not first else "below", lo_cnt if first else None):
                first = False
        states.append(st); tables.append(g.table()); pats.append("budget"); sts.append(skind)
    return dict(name=f"budget{mps}", mps=mps, opt=opt, chunk_start=0, supers=[[96, 64], [140]], budgets=budgets, states=states, tables=tables, patterns=pats,
                starts=sts)


@functools.lru_cache(maxsize=None)
def carried_case(mps):
    """a super-chunk in the middle of a run: chunk_start > 0, every pair carries a state"""
    return make_case(f"carried{mps}", mps, SAMPLE_OF[mps], _opt(SAMPLE_OF[mps], 5000, 1200), 1000, [[100, 157]], 64, 400 + mps, starts=("carried", "inactive", "empty"),
                     distinct=16)


STOP_CLAIMS = ("between", "on_trigger", "after_trigger", "trigger_on_bound", "at_max", "nowhere", "prob_one", "prob_above_one", "mult_zero", "mult_minus_one",
               "dyn_m1_no_trigger", "min_is_max_u64", "max_zero", "ratio_high", "ratio_low")


def case_list():
    """(name, claim or None, factory) of every case of the suite, smallest first; nothing is generated before a factory is called"""
    out = []
    for mps in (4, 12, 16):
        out += [(f"edge{mps}_{ln}", None, functools.partial(edge_case, mps, ln)) for ln in EDGE_LENS]
        out += [(f"multi{mps}_{w}", None, functools.partial(multi_case, mps, w)) for w in MULTI]
        out += [(f"carried{mps}", None, functools.partial(carried_case, mps)), (f"budget{mps}", None, functools.partial(budget_case, mps))]
        out += [(f"long{mps}_{ln}", None, functools.partial(long_case, mps, ln)) for ln in LONG_LENS]
    for ssz in (3, 5, 7):
        out += [(f"stop{ssz}_{claim}", claim, functools.partial(lambda s, i: stop_cases(s)[i][0], ssz, i)) for i, claim in enumerate(STOP_CLAIMS)]
    return out


def all_cases():
    """every case, generated: (case, claim or None)"""
    out = []
    for name, claim, make in case_list():
        case = make()
        assert case["name"] == name, (case["name"], name)
        out.append((case, claim))
    return out


_EXPECTED = {}


def expected(case):
    """the yardstick over the case's chain: per super-chunk, per pair, replay_ref.super_chunk's dict (the state of one super-chunk feeds the next)"""
    if case["name"] not in _EXPECTED:
        out, states, c0 = [], [dict(s) for s in case["states"]], case["chunk_start"]
        for lens in case["supers"]:
            res = [rr.super_chunk(t, s, case["opt"], c0, lens, case["budgets"] or ()) for s, t in zip(states, case["tables"])]
            out.append(res)
            states, c0 = [r["state"] for r in res], c0 + sum(lens)
        _EXPECTED[case["name"]] = out
    return _EXPECTED[case["name"]]


def stop_position(res, c0, c1, opt):
    """where one pair's first stop lies relative to the record breakers of the super-chunk [c0, c1): one of STOP_POSITIONS, or None"""
    st = res["state"]
    scan = [t["iter"] for ch in res["chunk_triggers"] for t in ch]
    done = [t["iter"] for t in res["executed"]]
    if st["active"]:
        return "nowhere" if opt.min_iterations >= c1 else None
    s = st["iterations"]
    if s == opt.max_iterations:
        return "at_max" if c0 < s < c1 else None
    if s in scan and s not in done:
        return "on_trigger"
    if done and done[-1] == s - 1:
        return "after_trigger"
    if done and any(t > s for t in scan) and s - 1 not in scan:
        return "between"
    return None
