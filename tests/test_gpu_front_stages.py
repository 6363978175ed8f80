"""The stages a step launches IN FRONT of the sweeps — k_prep / kc_prep, k_samples / kc_samples<5|6|7>, k_solve<S> (256- and 64-lane workgroups, with
and without an LDS reservation), kc_solve5_null -> _reduce -> _roots, kc_solve<6-point>, kc_solve<7-point> — through mdrp_front_stages, which runs
the scheduler's own stage functions on a caller's chunk list, against tests/front_stages_ref.py: slot by slot, record by record.

Which samples are judged: all of them, except where the references themselves disagree (the oracle's solver against the host build of the device's
solver differ in count or by more than the tolerance) — on the sample formed from the device's records, or on the same sample formed from the records
as the definitions give them (tests/front_stages_cases.py definition_records: they differ from the device's by at most 2 ulp in the inverse lengths).
The second clause is there for one 5-point sample (n = 37, iteration 271 of seed 32): its third pose moves by 2.7e-6 when the bearings move by one
ulp, the oracle and the host build are 1.08e-6 apart on the definitions' records and within 1e-6 on the device's, the device's split chain 1.6e-6
from the oracle.  The share is capped at 1 % of a case's live iterations here and, on the CPU, in tests/test_front_stages_host.py.
Measured on an MI355X (live iterations of the longest chunk list, n_max = 300):
  p3p 0 of 2885, shift 0 of 2885, shared 0 of 2885, varying 0 of 2885, 5-point 4 of 2885, 7-point 0 of 2885 unjudged (n_max = 291, 640 iterations:
  0 everywhere but the 5-point solver's 1); P3P: 580 NaN models, 577 of them in the pair that never has a real pose
  6-point (no host build; against the oracle with the unit test's allowance): 0 count differences, 0 iterations with a solution beyond 1e-6 of 1000;
  the same samples through mdrp_classic_solver_batch give the scheduler's solutions on 1000 of 1000"""
import numpy as np
import pytest

import front_stages_cases as fc
import front_stages_ref as fr

pytestmark = pytest.mark.gpu

THREADS = (None, 64)  # MDRP_SAMPLE_THREADS unset | one wavefront: at N = 300 a step of 64 threads often sees no rejection (the first = nthreads - 1 commit)
CASES = [(k, s, ch, t) for k, s in fc.KINDS for ch in fc.chunk_lists(k) for t in THREADS]
_TABLES = {}  # (kind, shift, n_max, chunks) -> the sample tables of the first run: the same under both thread counts


def _id(k, s, ch, t=None):
    return f"{fc.kind_id(k, s)}-{'_'.join(map(str, ch))}" + (f"-threads{t}" if t else "")


def _run(monkeypatch, kind, shift, d, chunks, threads=None, resident=None, initial=False):
    from mdrp_amd import _capi as capi
    for knob, v in (("MDRP_SAMPLE_THREADS", threads), ("MDRP_SOLVE_RESIDENT", resident)):
        monkeypatch.delenv(knob, raising=False)
        if v is not None:
            monkeypatch.setenv(knob, str(v))
    for knob in ("MDRP_CHUNKS", "MDRP_LO_OVERLAP"):
        monkeypatch.delenv(knob, raising=False)
    ro, bo = fc.options(kind, shift, chunks, initial)
    cro, cbo = fc.capi_options(ro, bo)
    r = capi.default_handle(0).front_stages(kind, d["x1"], d["x2"], d["d1"], d["d2"], cro, cbo, chunks, n_per_pair=d["n"], cam1=d["cam1"], cam2=d["cam2"],
                                            slot_iters=sum(chunks) + fc.SPARE)
    return r, ro, bo


def _filled(a):
    from mdrp_amd import _capi as capi
    return bool((np.ascontiguousarray(a).view(np.uint8) == capi.FRONT_FILL).all())


def _within(dev, ref, r):
    """|dev - ref| <= r 2^-53 |ref| in extended precision (r = 0: equal)"""
    dev, ref = fr.LD(dev), fr.LD(ref)
    return bool(abs(dev - ref) <= r * fr.LD(2.0) ** -53 * abs(ref))


# ------------------------------------------------------------------------------------------------------------------------ prep
def check_prep(kind, d, ro, bo, r, corrupted=()):
    """every assertion on what k_prep / kc_prep leave; `corrupted`: pairs with planted records, of which only what the filters rely on is asserted"""
    B, n_max = d["x1"].shape[:2]
    K, G = fr.SAMPLE_SIZE[kind], (n_max + 15) // 16
    st, pts, frag = r["states"], r["pts"], r["rfrag"]
    assert frag.shape == (B, G, 64, 4)  # a pair's fragments start at pair * ceil(n_max / 16) * 64 lanes
    tables = {}
    for i in range(B):
        n = int(d["n"][i])
        table = tables.setdefault(n, len(tables))
        c1 = None if d["cam1"] is None else d["cam1"][i]
        c2 = None if d["cam2"] is None else d["cam2"][i]
        x1, x2, s = d["x1"][i, :n], d["x2"][i, :n], st[i]
        assert _filled(pts[i, n:]) and (r["dep"] is None or _filled(r["dep"][i, n:])), i
        if kind <= 2:  # dep equals the input bytes
            assert r["dep"][i, :n, 0].tobytes() == d["d1"][i, :n].tobytes() and r["dep"][i, :n, 1].tobytes() == d["d2"][i, :n].tobytes(), i
        p4 = pts[i, :n, :4]
        bad = fr.unusable_rows(p4) if n else np.zeros(0, dtype=bool)
        # ---- fragments: rows of unusable records and rows from n to the end of n's group are zero, later groups are not written
        blk, written = fr.fragments(p4, n, n_max)
        g_end = (n + 15) // 16 * 16
        rows = frag[i].reshape(G, 4, 16, 4)  # [group][block of 16 lanes][row][word]
        for rec in list(np.nonzero(bad)[0]) + list(range(n, g_end)):
            assert not rows[rec >> 4, :, rec & 15].any(), (i, rec)
        assert _filled(frag[i, g_end // 16:]), i
        # ---- the box covers every finite coordinate
        fin = np.where(np.isfinite(p4), np.abs(p4), 0.0)
        for q in range(4):
            assert s["box"][q] >= (fin[:, q].max() if n else 0.0), (i, q)
        if i in corrupted:
            assert bad.any(), i
            continue
        assert not bad.any(), i
        # ---- sums, records, fragments of a clean pair
        if kind in (0, 3):
            norm_dev, cen_dev = None, np.zeros(4)  # cen: what was subtracted — nothing the state names (calibrated), the principal points (5-point)
            (_, _, cx1, cy1), (_, _, cx2, cy2) = fr.intrinsics(c1), fr.intrinsics(c2)
            assert s["norm"] == 1.0 and s["cen"].tolist() == ([0.0] * 4 if kind == 0 else [cx1, cy1, cx2, cy2]), i
        else:
            cen_ref, mean_abs = fr.scale_and_centre(kind, x1, x2, c1)
            cen_dev, norm_dev = s["cen"].copy(), s["norm"]
            if kind == 5 and n:  # centroids: sums of terms of either sign, so the bound is relative to the mean magnitude of the terms
                for q in range(4):
                    assert abs(fr.LD(cen_dev[q]) - cen_ref[q]) <= fr.sum_bound(n) * mean_abs[q], (i, q)
            elif kind in (1, 2):
                assert not cen_dev.any(), i
            else:
                assert np.array_equal(cen_dev, cen_ref.astype(np.float64)), i  # (6-point: the caller's principal point; an empty 7-point pair: zero)
            if n:
                norm_ref = fr.norm_of(x1, x2, cen_dev)
                assert abs(fr.LD(norm_dev) - norm_ref) <= fr.sum_bound(n) * norm_ref, (i, norm_dev, norm_ref)
        if n:
            want = fr.points(kind, x1, x2, c1, c2, norm_dev, cen_dev)
            assert p4.tobytes() == want.tobytes(), (i, np.nonzero(p4 != want))
            inv = fr.inverse_lengths(p4)  # within 2 ulp: three roundings of positive partial sums halved by the root, the root's and the quotient's half ulp
            err = np.abs(pts[i, :n, 4:6].astype(fr.LD) - inv)
            assert (err <= 2 * np.spacing(inv.astype(np.float64)).astype(fr.LD)).all(), (i, float(err.max()))
            for q in range(4):
                assert s["box"][q] == np.abs(p4[:, q]).max(), (i, q)
            assert frag[i][written].tobytes() == blk[written].tobytes(), i
        # ---- thresholds and scales: within r 2^-53 of the defining expression; the exact fields
        if n or kind in (0, 3):
            for name, (val, rr) in fr.state_fields(kind, n, c1, c2, norm_dev if n else 1.0, ro, bo).items():
                if n or name != "norm":
                    assert _within(s[name], val, rr), (i, name, s[name], float(val), rr)
        exact, best = fr.exact_fields(kind, n, table, K, ro, s["sq_thr"])
        for name, val in exact.items():
            assert s[name] == val, (i, name, s[name], val)
        assert np.array_equal(np.ascontiguousarray(s["best"]).view(np.float64).reshape(12), best), i
        assert int(r["table_of_pair"][i]) == table
    assert r["table_n"].tolist() == list(tables), (r["table_n"], tables)


# ------------------------------------------------------------------------------------------------------------------------ sampler
def check_samples(kind, d, ro, chunks, r, key=None):
    K, total = fr.SAMPLE_SIZE[kind], sum(chunks)
    assert r["samples"].shape == (len(r["table_n"]), total, K)
    for t, n in enumerate(r["table_n"]):
        if n < K:  # a table with N < K is left untouched
            assert _filled(r["samples"][t]), t
        else:      # the chunks concatenated are the sequence for (seed, N, K)
            want = fr.draw_table(ro["seed"], int(n), K, total)
            assert np.array_equal(r["samples"][t].astype(np.int64), want), (t, n, np.nonzero((r["samples"][t] != want).any(axis=1))[0][:5])
    if key is not None:
        assert _TABLES.setdefault(key, r["samples"].tobytes()) == r["samples"].tobytes()


# ------------------------------------------------------------------------------------------------------------------------ solver
def check_slots(kind, shift, d, chunks, r, judge=True, definition=None):
    """the slot tables, tag lists and counters of every chunk; judge: also the solutions against the oracle.  Returns the counts printed by the test"""
    from mdrp_amd import _capi as capi
    name, K, mps = fr.solver_name(kind, shift), fr.SAMPLE_SIZE[kind], fr.MODEL_SLOTS[kind]
    B, total = len(d["n"]), sum(chunks)
    inl, models, tags, mc = r["slot_inl"], r["models"], r["tags"], r["model_count"]
    assert inl.shape == (len(chunks), B, total + fc.SPARE, mps)
    stat = dict(live=0, unjudged=0, count_diff=0, loose=0, nan=0, six_inputs=[], six_rows=[], wrong=[])
    for p in range(B):
        n = int(d["n"][p])
        if n < K:  # the inactive pair: every slot, tag and model keeps the fill pattern, nothing is counted
            assert _filled(inl[:, p]) and _filled(models[p]) and _filled(tags[:, p]) and not mc[:, p].any(), p
            continue
        table = int(r["table_of_pair"][p])
        final = inl[-1, p]
        for c, (off, length) in enumerate(fc.chunk_of(chunks)):
            # behind chunk c: its iterations and those before it are written (and stay as they were), everything behind them keeps the fill pattern
            assert np.array_equal(inl[c, p, :off + length], final[:off + length]) and _filled(inl[c, p, off + length:]), (p, c)
            live = np.argwhere(final[off:off + length] == -2)
            want = np.sort((live[:, 0] + off) * mps + live[:, 1]).astype(np.uint32)
            assert mc[c, p, 0] == len(want) and mc[c, p, 1] == 0, (p, c, mc[c, p], len(want))
            assert np.array_equal(np.sort(tags[c, p, :len(want)]), want) and _filled(tags[c, p, len(want):]), (p, c)
        assert _filled(models[p, total:]) and np.isin(final[:total], (-1, -2, -3)).all() and not (final[:total, 1:] == -3).any(), p
        counts = (final[:total] == -2).sum(axis=1)
        if name != "5pt":  # the -2 / -1 pattern of the solution count; a 5-point pose sits in slot `root index` of its iteration
            assert ((final[:total] == -2) == (np.arange(mps)[None, :] < counts[:, None])).all(), p
        if not judge:
            continue
        refs = fc.pair_references(kind, shift, r["pts"][p], None if r["dep"] is None else r["dep"][p], r["samples"][table])
        if definition is not None:  # ... and on the records as the definitions give them: a sample is judged where the references agree on both
            dpts, ddep = definition
            twin = fc.pair_references(kind, shift, dpts[p], ddep[p] if kind <= 2 else None, r["samples"][table])
            refs = [(a[0], a[1], a[2] and b[2], a[3]) for a, b in zip(refs, twin)]
        pred = np.array([x[3] for x in refs], dtype=bool)
        for it, (orc, host, judged, _) in enumerate(refs):
            stat["live"] += 1
            mine = [row for row, s in zip(fr.device_rows(name, models[p, it]), final[it]) if s == -2]
            if name == "6pt":  # no host build: against the oracle, with the allowance of the unit test; in the oracle's order
                stat["count_diff"] += len(mine) != len(orc)
                stat["loose"] += len(mine) == len(orc) and not fr.same_solutions(name, mine, orc, ordered=True)
                stat["six_inputs"].append(fr.solver_inputs(kind, r["pts"][p][r["samples"][table][it].astype(np.int64)], None)[:2])
                stat["six_rows"].append(mine)
                continue
            if not judged:
                stat["unjudged"] += 1
                continue
            if len(mine) != len(orc) or not fr.same_solutions(name, mine, orc, ordered=name == "7pt"):
                stat["wrong"].append((p, it, len(mine), len(orc)))
        if name == "p3p":
            nan = final[:total, 0] == -3
            stat["nan"] += int(nan.sum())
            must = np.zeros(total, dtype=bool)
            must[fc.nan_front(counts, pred, chunks)] = True
            # -3: the reference's P3P answers the sample with NaN poses, the device has no solution for it, the slot holds a NaN model — and every
            # such iteration in front of the first real pose of its wavefront has it (behind that pose the slot is empty: the record stands)
            assert np.array_equal(nan, must), (p, np.nonzero(nan != must)[0][:8])
            assert not (nan & (counts > 0)).any() and pred[nan].all()
            for it in np.nonzero(nan)[0]:
                m = models[p, it, 0]
                assert np.isnan(m["q"]).all() and np.isnan(m["t"]).all() and np.isnan(m["scale"]), (p, it)
    return stat


def _print_and_cap(name, chunks, stat):
    print(f"{name} {chunks}: {stat['unjudged']} of {stat['live']} live iterations unjudged" +
          (f"; 6-point: {stat['count_diff']} count differences, {stat['loose']} iterations with a solution beyond 1e-6" if name == "6pt" else "") +
          (f"; {stat['nan']} NaN models" if name == "p3p" else ""))
    assert not stat["wrong"], (name, "(pair, iteration, solutions, the oracle's)", stat["wrong"])
    assert stat["unjudged"] <= fc.UNJUDGED_CAP * stat["live"], (stat["unjudged"], stat["live"])
    assert stat["count_diff"] <= fc.SIXPT_CAP * stat["live"] and stat["loose"] <= fc.SIXPT_CAP * stat["live"], (stat["count_diff"], stat["loose"], stat["live"])


def _six_second_witness(stat):
    """the same samples through mdrp_classic_solver_batch (the one-kernel unit path): printed, not asserted"""
    from mdrp_amd import _capi as capi
    a = np.stack([x[0] for x in stat["six_inputs"]])
    b = np.stack([x[1] for x in stat["six_inputs"]])
    out, n = capi.default_handle(0).classic_solver_batch(capi.SHARED_6PT, a, b)
    same = sum(fr.same_solutions("6pt", fr.device_rows("6pt", out[i][:n[i]]), stat["six_rows"][i], ordered=True) for i in range(len(n)))
    print(f"6pt: mdrp_classic_solver_batch gives the scheduler's solutions on {same} of {len(n)} samples")


# ------------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("kind,shift,chunks,threads", CASES, ids=[_id(*c) for c in CASES])
def test_front_stages(monkeypatch, kind, shift, chunks, threads):
    d = fc.batch(kind, shift, fc.N_MAX)
    r, ro, bo = _run(monkeypatch, kind, shift, d, chunks, threads=threads)
    check_prep(kind, d, ro, bo, r)
    check_samples(kind, d, ro, chunks, r, key=(kind, shift, fc.N_MAX, chunks))
    stat = check_slots(kind, shift, d, chunks, r, definition=fc.definition_records(kind, shift, fc.N_MAX))
    _print_and_cap(fr.solver_name(kind, shift), chunks, stat)
    if kind == 4 and chunks == fc.chunk_lists(4)[-1] and threads is None:
        _six_second_witness(stat)
    if (kind, shift) == (0, False) and chunks == fc.CHUNK_LISTS[-1]:
        assert stat["nan"] >= 5, stat["nan"]  # the inputs hold what the -3 rule is checked on


@pytest.mark.parametrize("chunks", fc.CHUNK_LISTS, ids=["_".join(map(str, c)) for c in fc.CHUNK_LISTS])
def test_front_stages_with_a_solver_reservation(monkeypatch, chunks):
    """calibrated P3P under MDRP_SOLVE_RESIDENT: the second chunk of a pipelined list is solved by one-wavefront workgroups with an LDS reservation
    (the NaN predicate's wavefront is then the workgroup) — the same slots"""
    d = fc.batch(0, False, fc.N_MAX)
    r, ro, bo = _run(monkeypatch, 0, False, d, chunks, resident=2)
    check_samples(0, d, ro, chunks, r, key=(0, False, fc.N_MAX, chunks))
    _print_and_cap("p3p", chunks, check_slots(0, False, d, chunks, r, definition=fc.definition_records(0, False, fc.N_MAX)))
    plain, _, _ = _run(monkeypatch, 0, False, d, chunks)
    assert r["slot_inl"].tobytes() == plain["slot_inl"].tobytes() and r["models"].tobytes() == plain["models"].tobytes()
    assert np.array_equal(r["model_count"], plain["model_count"])


@pytest.mark.parametrize("kind,shift", fc.KINDS, ids=[fc.kind_id(k, s) for k, s in fc.KINDS])
def test_front_stages_at_an_odd_width_with_an_initial_model(monkeypatch, kind, shift):
    """n_max = 291: the last fragment group holds three rows; score_initial_model: the records a run starts from"""
    chunks = fc.chunk_lists(kind)[1]
    d = fc.batch(kind, shift, fc.N_MAX_ODD)
    r, ro, bo = _run(monkeypatch, kind, shift, d, chunks, initial=True)
    assert ro["score_initial_model"] and int(r["states"]["refinements"].sum()) == (0 if kind == 5 else 5)
    check_prep(kind, d, ro, bo, r)
    check_samples(kind, d, ro, chunks, r)
    _print_and_cap(fr.solver_name(kind, shift), chunks, check_slots(kind, shift, d, chunks, r, definition=fc.definition_records(kind, shift, fc.N_MAX_ODD)))


def test_corrupted_records_touch_nothing_else(monkeypatch):
    """a NaN, an inf and 1e16 in three pairs of a calibrated batch: zero fragment rows, a box that covers every finite coordinate, and the clean pair
    of the batch — its records, fragments, state, slots, models and tags — byte for byte what it is without them"""
    chunks = (65, 3)
    bad, clean = fc.corrupted_batch(), fc.corrupted_batch(False)
    r, ro, bo = _run(monkeypatch, 0, False, bad, chunks)
    check_prep(0, bad, ro, bo, r, corrupted=tuple(fc.CORRUPT))
    for pair, rows in fc.CORRUPT_ZERO_ROWS.items():
        flagged = np.nonzero(fr.unusable_rows(r["pts"][pair, :, :4]))[0].tolist()
        assert flagged == list(rows), (pair, flagged)
    check_samples(0, bad, ro, chunks, r)
    check_slots(0, False, bad, chunks, r, judge=False)
    want, _, _ = _run(monkeypatch, 0, False, clean, chunks)
    check_prep(0, clean, ro, bo, want)
    for name in ("pts", "dep", "rfrag", "states", "models"):
        assert r[name][0].tobytes() == want[name][0].tobytes(), name
    for name in ("slot_inl", "tags", "model_count"):
        assert r[name][:, 0].tobytes() == want[name][:, 0].tobytes(), name
    assert r["samples"].tobytes() == want["samples"].tobytes()


def test_sample_tables_meet_the_golden_sampler(monkeypatch, golden):
    """K = 3 at an (N, seed) of tests/golden/sampler.npz (the reference binary's own sequence): N = 200 and N = 7 with seed 5, two chunks"""
    from mdrp_amd import _capi as capi
    g = golden("sampler")
    d = fc.batch(1, False, fc.N_MAX)
    d = dict(d, x1=d["x1"][:2, :200], x2=d["x2"][:2, :200], d1=d["d1"][:2, :200], d2=d["d2"][:2, :200], n=np.array([200, 7], dtype=np.int32))
    for threads in THREADS:
        monkeypatch.delenv("MDRP_SAMPLE_THREADS", raising=False)
        if threads:
            monkeypatch.setenv("MDRP_SAMPLE_THREADS", str(threads))
        ro, bo = fc.options(1, False, (63, 1))
        cro, cbo = fc.capi_options(dict(ro, seed=5), bo)
        r = capi.default_handle(0).front_stages(1, d["x1"], d["x2"], d["d1"], d["d2"], cro, cbo, (63, 1), n_per_pair=d["n"])
        assert r["table_n"].tolist() == [200, 7]
        assert np.array_equal(r["samples"][0], g["n200_s5"]) and np.array_equal(r["samples"][1], g["n7_s5"]), threads


def test_refusals_before_any_device_work():
    """a chunk list the pass's scratch layout cannot hold is MDRP_ERR_INVALID — the 5-point first chunk's Reduce5 region included — and the handle stays usable"""
    from mdrp_amd import _capi as capi
    h = capi.Handle(0)
    try:
        for kind, chunks, spare, what in ((0, (4, 5), -1, "capacity"), (0, (), 0, "1 to 8 chunks"), (0, (1,) * 9, 0, "1 to 8 chunks"), (0, (3, 0), 0, "length < 1"),
                                          (3, (129, 300), 0, "Reduce5")):
            d = fc.batch(kind, False, fc.N_MAX)
            ro, bo = fc.options(kind, False, chunks)
            cro, cbo = fc.capi_options(dict(ro, max_iterations=max(sum(chunks), 1) + spare, min_iterations=max(sum(chunks), 1) + spare), bo)
            with pytest.raises(capi.MdrpError, match=what):
                h.front_stages(kind, d["x1"], d["x2"], d["d1"], d["d2"], cro, cbo, chunks, n_per_pair=d["n"], cam1=d["cam1"], cam2=d["cam2"],
                               slot_iters=max(sum(chunks), 1))
        d = fc.batch(3, False, fc.N_MAX)
        ro, bo = fc.options(3, False, (128, 301))
        r = h.front_stages(3, d["x1"], d["x2"], None, None, *fc.capi_options(ro, bo), (128, 301), n_per_pair=d["n"], cam1=d["cam1"], cam2=d["cam2"])
        assert (r["model_count"][:, :4, 0] > 0).all() and not r["model_count"][:, 5].any()
    finally:
        h.close()
