"""The calls of the history matrix for the entry points of include/mdrp_classic_frontend.h (a helper, not a test): the tables of
tests/history_cases.py, tests/classic_history_cases.py and tests/classic_models_history_cases.py enumerate the handle entry points of the other
three headers; the baselines' device front end is declared in its own extension header and has its calls here, built from the same classes, and
tests/test_gpu_classic_frontend_history.py runs them against those tables in both directions.  The new calls gather into the buffers the
monodepth front end gathers into (fe_x1, fe_x2, fe_slot, fe_n, fe_key), so the monodepth front-end calls are among the predecessors."""
import functools
import os
import re

import numpy as np

import history_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = ([(1, None), (2, None), (3, None), (63, None), (64, None), (300, None)], [(255, None), (256, None), (257, None), (70, None), (100, None), (2, None)])
ITERATIONS = {3: 200, 4: 64, 5: 200}


class PointMatches(hc.Matches):
    """mdrp_gather_point_matches(_ranked) / mdrp_estimate_classic_matches(_ranked)_async on a batch of tests/classic_frontend_cases.py (float32
    tables, int64 matches); kind 3: cameras, kind 4: the principal point and centred keypoints, kind 5: neither"""
    family = "classic_front_end"
    progressive = None  # ranked estimates: ropt.progressive_sampling as the caller spells it (None: absent)

    def make(self):
        import classic_frontend_cases as cf
        import frontend_ranked_cases as rc
        b = dict(cf.make_batch(SPECS[self.which], 200 + 20 * self.which))
        if self.kind == 4:
            b = cf.shared_focal_tables(b)
        if self.score_dtype is not None:
            b["scores"] = rc.batch_scores(cf.kept_rows(b), 2, 5).astype(self.score_dtype)
        return b

    def digest_arrays(self, d):
        return [d["kp1"], d["kp2"], d["matches"]] + ([d["scores"]] if "scores" in d else [])

    def centred(self):
        return self.kind == 4

    def descriptor(self):
        """(mdrp_point_matches, B, M, score pointer) over tensors uploaded once"""
        key = self.name + "/descriptor"
        if key not in hc._DEV:
            import mdrp_amd.poselib as poselib
            d = self.data()
            t = hc.device_arrays(self.name, [d["kp1"].astype(np.float32), d["kp2"].astype(np.float32), d["matches"]] + ([d["scores"]] if "scores" in d else []))
            pm, keep, B, M, _ = poselib._point_matches_descriptor(*t[:3], d["c1"] if self.centred() else None, d["c2"] if self.centred() else None)
            hc._torch().cuda.synchronize()  # (the descriptor's own copies: matches narrowed to int32, the centres)
            hc._DEV[key] = (pm, B, M, t[3].data_ptr() if len(t) > 3 else None, keep)
        return hc._DEV[key][:4]

    def pair_cameras(self, B):
        import mdrp_amd.poselib as poselib
        import test_gpu_frontend as fe
        if self.kind == 3:
            return poselib._camera_records(fe.CAM1, B), poselib._camera_records(fe.CAM2, B)
        if self.kind == 4:
            rec = poselib._pp_records(None, B)[0]
            return rec, rec
        return None, None

    def ransac_options(self):
        import test_gpu_frontend as fe
        it = ITERATIONS.get(self.kind, 200)  # (a refusal's spoiled kind has no entry)
        ro = dict(fe.RO, max_iterations=it, min_iterations=it, max_prosac_iterations=150)
        if self.progressive is not None:
            ro["progressive_sampling"] = self.progressive
        return ro

    def run(self, h):
        capi = hc._capi()
        desc, B, M, sp = self.descriptor()
        ranked = self.score_dtype is not None
        torch = hc._torch()
        if not self.estimate:
            out = [hc.device_out((B, M, 2), torch.float64), hc.device_out((B, M, 2), torch.float64), hc.device_out((B, M), torch.int32)]
            n = h.gather_points(desc, B, *[t.data_ptr() for t in out], sp, self.score_type(), ranked)
            h.synchronize()
            return tuple(hc.host_bytes(t) for t in out) + (n.tobytes(),)
        import test_gpu_frontend as fe
        ro, bo = capi.ransac_opt_from_dict(self.ransac_options()), capi.bundle_opt_from_dict(fe.BO)
        cam1, cam2 = self.pair_cameras(B)
        mask = hc.device_out((B, M), torch.uint8, hc.FILL)
        n = h.estimate_points_device(self.kind, desc, B, ro, bo, cam1, cam2, mask.data_ptr(), sp, self.score_type(), ranked)
        records = h.fetch_results(B).tobytes()
        self.stats = h.last_stats()
        return records, hc.host_bytes(mask), n.tobytes()

    @property
    def outputs(self):
        return ("records", "match mask", "n") if self.estimate else ("x1", "x2", "slot", "n")


class PointImagePairs(PointMatches):
    """the same four on per-image tables (tests/classic_frontend_cases.image_batch)"""

    def make(self):
        import classic_frontend_cases as cf
        import frontend_ranked_cases as rc
        b = dict(cf.image_batch())
        if self.score_dtype is not None:
            b["scores"] = rc.batch_scores(cf.image_kept_rows(b), 3, 12).astype(self.score_dtype)
        return b

    def digest_arrays(self, d):
        return [d["keypoints"], d["pairs"], d["matches"], d["kp_counts"], d["centers"]] + ([d["scores"]] if "scores" in d else [])

    def descriptor(self):
        key = self.name + "/descriptor"
        if key not in hc._DEV:
            import mdrp_amd.poselib as poselib
            d = self.data()
            t = hc.device_arrays(self.name, [d["keypoints"].astype(np.float32), d["matches"]] + ([d["scores"]] if "scores" in d else []))
            desc, keep, host_pairs, B, M, I, _ = poselib._point_image_pairs_descriptor(t[0], d["pairs"], t[1], d["centers"] if self.centred() else None,
                                                                                      d["kp_counts"], True)
            hc._torch().cuda.synchronize()
            hc._DEV[key] = (desc, B, M, t[2].data_ptr() if len(t) > 2 else None, keep, host_pairs, I)
        return hc._DEV[key][:4]

    def pair_cameras(self, B):
        import image_pairs_cases as ipc
        import mdrp_amd.poselib as poselib
        if self.kind == 3:
            host_pairs, I = hc._DEV[self.name + "/descriptor"][5:7]
            return poselib._pair_cameras(ipc.CAMERAS, host_pairs, I)
        return PointMatches.pair_cameras(self, B)


FETCH = "mdrp_fetch_results"


@functools.lru_cache(maxsize=None)
def probes():
    """every entry point of the header, the per-pair and the per-image form each with float32 and float64 scores, every kind, both batches of SPECS"""
    m, ip = PointMatches, PointImagePairs
    f32, f64 = np.float32, np.float64
    return (
        m("gather_point_matches", ["mdrp_gather_point_matches"], kind=5, which=0),
        m("gather_point_matches_ranked_f32", ["mdrp_gather_point_matches_ranked"], kind=5, score_dtype=f32),
        m("estimate_classic_matches_5pt", ["mdrp_estimate_classic_matches_async", FETCH], kind=3, estimate=True),
        m("estimate_classic_matches_ranked_7pt_f32", ["mdrp_estimate_classic_matches_ranked_async", FETCH], kind=5, estimate=True, score_dtype=f32, which=0),
        m("estimate_classic_matches_ranked_6pt_f64", ["mdrp_estimate_classic_matches_ranked_async", FETCH], kind=4, estimate=True, score_dtype=f64, progressive=True),
        ip("gather_point_image_pairs", ["mdrp_gather_point_image_pairs"], kind=4),
        ip("gather_point_image_pairs_ranked_f64", ["mdrp_gather_point_image_pairs_ranked"], kind=5, score_dtype=f64),
        ip("estimate_classic_image_pairs_7pt", ["mdrp_estimate_classic_image_pairs_async", FETCH], kind=5, estimate=True),
        ip("estimate_classic_image_pairs_ranked_5pt_f64", ["mdrp_estimate_classic_image_pairs_ranked_async", FETCH], kind=3, estimate=True, score_dtype=f64,
           progressive=False),
    )


def by_name(name):
    return next(c for c in probes() if c.name == name)


@functools.lru_cache(maxsize=None)
def refusals():
    """calls the new entry points refuse before any device work: a monodepth kind, a NULL matches pointer, a score type that is none"""
    return (hc.Refusal("refused_classic_matches_kind", by_name("estimate_classic_matches_5pt"), hc._spoil_attr("kind", 0)),
            hc.Refusal("refused_classic_matches_null", by_name("estimate_classic_matches_ranked_7pt_f32"), hc._spoil_descriptor("matches", None)),
            hc.Refusal("refused_classic_image_pairs_score_type", by_name("gather_point_image_pairs_ranked_f64"), hc._spoil_attr("score_type_override", 2)))


# the predecessors out of the other tables: a larger and a smaller call, other kinds, host and device buffers, the monodepth front end in every form
# (the gather buffers and the key scratch are shared with it), a refused front-end call, a ranked baseline
PREDECESSORS = ("larger_k3", "below_every_probe", "k0_device", "k5_host", "k4_device", "gather_matches", "estimate_matches", "estimate_matches_ranked_float32",
                "gather_matches_ranked_float64", "gather_image_pairs", "estimate_image_pairs", "estimate_image_pairs_ranked_float64", "refused_matches")
# the probes of the other tables run behind every new call: the monodepth front end in every form, plain and ranked estimates of the baselines' kinds
FOLLOWERS = ("gather_matches", "estimate_matches", "gather_matches_ranked_float32", "estimate_matches_ranked_float64", "gather_image_pairs", "estimate_image_pairs",
             "gather_image_pairs_ranked_float64", "estimate_image_pairs_ranked_float32", "k3_device", "k5_host", "k4_host", "k0_device")


def predecessors():
    import classic_history_cases as chc
    ranked = tuple(c for c in chc.probes() if c.name == "classic_ranked_device_150")
    return tuple(hc.by_name(n) for n in PREDECESSORS) + ranked + probes() + refusals()


def followers():
    import classic_history_cases as chc
    return tuple(hc.by_name(n) for n in FOLLOWERS) + tuple(c for c in chc.probes() if c.name in ("classic_ranked_device_150", "classic_ranked_host_presorted"))


def extension_entry_points():
    """names of the functions declared in include/mdrp_classic_frontend.h with an `mdrp_handle *` parameter (tests/test_history_host.py's parse)"""
    src = open(os.path.join(ROOT, "include", "mdrp_classic_frontend.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = "\n".join(line for line in src.splitlines() if not line.lstrip().startswith("#"))
    decls = re.findall(r"\b(mdrp_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S)
    return sorted({name for name, args in decls if re.search(r"\bmdrp_handle\s*\*\s*\w", args)})
