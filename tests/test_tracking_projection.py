"""The tracking thread's matchers with the projection on the device (pgorb_search_local_points, pgorb_search_by_projection_last_frame,
pgorb_search_by_projection_keyframe_pose and their *_batch_device forms; pilotguru_amd/csrc/track.hip) against the plain reference
of tests/tracking_reference.py on the constructed scenes of tests/tracking_cases.py.

On the CPU: the scenes reach every edge the reference counts, every mutant of the reference changes a compared output on them,
the reference's matching equals tests/matcher_reference.py fed with the reference's own front part, and malformed input is
refused before a device is needed.  On the GPU: integers equal the reference, floats equal it as bit patterns (the contract is a
fixed operation sequence, so there is no tolerance), single calls equal batches, streams and repeats give the same bytes."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matcher_reference as R  # noqa: E402
import tracking_cases as TC  # noqa: E402
import tracking_reference as TR  # noqa: E402
from matcher_cases import SF  # noqa: E402

_CACHE = {}


def singles():
    if "singles" not in _CACHE:
        _CACHE["singles"] = TC.single_cases()
    return _CACHE["singles"]


def batches():
    if "batches" not in _CACHE:
        _CACHE["batches"] = TC.batches()
    return _CACHE["batches"]


def all_cases():
    return singles() + [c for b in batches() for _, _, c in b.pairs]


def want(c):
    """The reference's result and hits of a case, computed once per session and not changed afterwards."""
    if c.name not in _CACHE:
        h = collections.Counter()
        _CACHE[c.name] = (TC.run_reference(c, hits=h), h)
    return _CACHE[c.name][0]


SINGLE_NAMES = ["local_edges", "local_scene", "local_th5", "local_nothing_to_match", "last_edges", "last_scene", "last_axis_no_ori",
                "kf_edges", "kf_scene", "kf_axis_th3"]
BATCH_KINDS = ["local", "last", "kf"]


def single(name):
    return [c for c in singles() if c.name == name][0]


def batch(kind):
    return [b for b in batches() if b.kind == kind][0]


# ---------------------------------------------------------------- CPU
def test_case_lists_are_what_the_tests_name():
    assert [c.name for c in singles()] == SINGLE_NAMES and [b.kind for b in batches()] == BATCH_KINDS
    big = single("local_scene")
    assert TC.BOUNDS[1] - TC.BOUNDS[0] == 640 and TC.BOUNDS[3] - TC.BOUNDS[2] == 480 and len(SF) == 9
    assert 380 <= len(big.keys) <= 420 and len(big.points) == 300
    assert {single("local_edges").th, single("local_th5").th} == {1.0, 5.0}
    for b in batches():
        assert len(b.frames) == 3 and len(b.pairs) == 4 and b.qcap % 64 != 0
        assert len({f for f, _, _ in b.pairs}) < 4                                           # two pairs share a frame
        assert all(c.points is b.points for _, _, c in b.pairs)                              # one table
        nq = [len(c.queries) if b.kind == "local" else len(c.other_keys) for _, _, c in b.pairs]
        assert 0 in nq and b.qcap in nq


EDGES = {
    "local": ["z_neg_zero", "z_pos_zero", "z_tiny", "z_negative", "nan_projection", "inf_projection",
              "u_min_on", "u_max_on", "v_min_on", "v_max_on", "u_min_ulp_below", "u_max_ulp_above", "v_min_ulp_below", "v_max_ulp_above",
              "dist_min_on", "dist_min_ulp_below", "dist_min_ulp_above", "dist_max_on", "dist_max_ulp_below", "dist_max_ulp_above",
              "depth_low", "depth_high", "viewcos_limit_on", "viewcos_limit_ulp_below", "viewcos_low", "viewcos_above_0998",
              "viewcos_below_0998", "predict_scale_clamped_low", "predict_scale_clamped_high", "slot_bad", "bad_slot_keypoint_taken",
              "slot_seen", "query_in_slot", "query_seen_flag", "query_bad", "n_to_match_zero", "candidate_blocked", "outside_bounds"],
    "last": ["last_null", "last_outlier", "last_bad", "last_bad_matched", "invz_negative", "z_neg_zero", "z_pos_zero", "z_tiny",
             "nan_projection", "u_min_on", "u_max_on", "v_min_on", "v_max_on", "u_min_ulp_below", "u_max_ulp_above", "v_min_ulp_below",
             "v_max_ulp_above", "outside_bounds", "candidate_blocked", "hist_kept_bins"],
    "kf": ["kf_null", "kf_bad", "kf_found", "behind_camera_matched", "z_neg_zero", "z_pos_zero", "z_negative", "nan_projection",
           "inf_projection", "u_min_on", "u_max_on", "v_min_on", "v_max_on", "u_min_ulp_below", "u_max_ulp_above", "v_min_ulp_below",
           "v_max_ulp_above", "dist_min_on", "dist_min_ulp_below", "dist_min_ulp_above", "dist_max_on", "dist_max_ulp_below",
           "dist_max_ulp_above", "predict_scale_clamped_low", "predict_scale_clamped_high", "candidate_blocked", "hist_kept_bins"],
}


@pytest.mark.parametrize("kind", BATCH_KINDS)
def test_cases_reach_every_edge(kind):
    hits = collections.Counter()
    for c in all_cases():
        if c.kind == kind:
            want(c)
            hits.update(_CACHE[c.name][1])
    missing = [k for k in EDGES[kind] if hits[k] == 0]
    assert not missing, "%s: edges never reached: %s" % (kind, missing)


def test_edge_scenes_hold_the_named_edges_themselves():
    """The constructed edges are in the edge scenes (identity pose, exactly representable inputs), not an accident of a generic one."""
    for name, kind in (("local_edges", "local"), ("last_edges", "last"), ("kf_edges", "kf")):
        want(single(name))
        h = _CACHE[name][1]
        for k in EDGES[kind]:
            if k.startswith(("u_m", "v_m", "dist_m", "z_neg_zero", "z_pos_zero", "z_tiny", "nan_", "viewcos_limit", "predict_scale_clamped")):
                assert h[k] > 0, (name, k)


@pytest.mark.parametrize("mutant", sorted(TR.MUTANTS))
def test_every_mutant_changes_a_compared_output(mutant):
    changed = [c.name for c in all_cases() if TC.differences(c.kind, want(c), TC.run_reference(c, TR.MUTANTS[mutant]))]
    assert changed, "no case tells %s from the reference" % mutant


@pytest.mark.parametrize("name", SINGLE_NAMES)
def test_reference_matching_equals_matcher_reference_on_its_own_front_part(name):
    c = single(name)
    w = want(c)
    f = w["front"]
    if c.kind == "local":
        got = R.search_by_projection_points(c.keys, c.desc, TC.BOUNDS, SF, f["kp_has_point"], f["valid"], f["proj_x"], f["proj_y"], f["level"],
                                            f["view_cos"], f["pdesc"], f["pobs"], c.th, c.nnratio)
    elif c.kind == "last":
        got = R.search_by_projection_frame(c.keys, c.desc, TC.BOUNDS, SF, c.has, f["valid"], f["u"], f["v"], f["last_octave"],
                                           f["last_angle"], f["pdesc"], f["pobs"], c.th, c.ori)
    else:
        got = R.search_by_projection_keyframe(c.keys, c.desc, TC.BOUNDS, SF, c.has, f["valid"], f["found"], f["u"], f["v"], f["dist3d"],
                                              f["min_distance"], f["max_distance"], TC.log_sf(), f["kf_angle"], f["pdesc"], c.th, c.orb_dist,
                                              c.ori, TR._LOG_F())
    assert got[0] == w["nmatches"] and np.array_equal(got[1], w["assigned"])


NEW_SYMBOLS = ["pgorb_search_local_points", "pgorb_search_by_projection_last_frame", "pgorb_search_by_projection_keyframe_pose"]


def test_symbols_and_methods_exist():
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and hasattr(L, s + "_batch_device") and s in _lib.SYMBOLS
    for m in ("SearchLocalPoints", "SearchByProjectionLastFramePose", "SearchByProjectionKeyFramePose"):
        assert callable(getattr(pg.ORBmatcher, m))


class _HostFrame:
    """A frame without a device (ext is None): the wrappers' own checks come before any library call."""

    def __init__(self, c):
        self.ext, self.N, self.bounds = None, len(c.keys), TC.BOUNDS
        self.mvKeys = self.mvKeysUndistorted = c.keys
        self.mDescriptors = c.desc


def _wrapper_call(c, **over):
    import pilotguru_amd as pg
    pts, pd, bad, obs = TC.table_arrays(c.points)
    T = pg.MapPointTable(pts, pd, bad, np.zeros(len(pts) + 1, np.int32), np.zeros(0, np.uint64))
    a = dict(th=c.th, bounds=None, idx=c.queries if c.kind == "local" else c.other_point, slots=c.slots)
    a.update(over)
    m, F = pg.ORBmatcher(0.8, True), _HostFrame(c)
    if c.kind == "local":
        return m.SearchLocalPoints(F, c.pose, a["slots"], T, a["idx"], c.query_seen if len(a["idx"]) == len(c.queries) else None, a["th"],
                                   bounds=a["bounds"], point_has_obs=obs)
    if c.kind == "last":
        return m.SearchByProjectionLastFramePose(F, c.pose, c.other_keys, a["idx"], T, a["th"], c.flag, c.has, bounds=a["bounds"], point_has_obs=obs)
    return m.SearchByProjectionKeyFramePose(F, c.pose, c.other_keys, a["idx"], T, a["th"], c.orb_dist, c.flag, c.has, bounds=a["bounds"])


def _bad_inputs(c):
    """(name, overrides) the calls must refuse: an index out of range, th <= 0, empty bounds, and for the local points a repeated
    query, a NULL query and a slot out of range."""
    n, idx = len(c.points), c.queries if c.kind == "local" else c.other_point
    hi, lo = idx.copy(), idx.copy()
    hi[0], lo[0] = n, -2
    bad = [("index == npoints", dict(idx=hi)), ("index < -1", dict(idx=lo)), ("th == 0", dict(th=0.0)), ("th < 0", dict(th=-1.0)),
           ("max_x == min_x", dict(bounds=(1.0, 1.0, 0.0, 2.0))), ("max_y < min_y", dict(bounds=(0.0, 2.0, 3.0, 1.0)))]
    if c.kind == "local":
        rep, null, sl = idx.copy(), idx.copy(), c.slots.copy()
        rep[1], null[0], sl[0] = rep[0], -1, n
        bad += [("a repeated query", dict(idx=rep)), ("a NULL query", dict(idx=null)), ("a slot out of range", dict(slots=sl))]
    return bad


@pytest.mark.parametrize("name", ["local_th5", "last_axis_no_ori", "kf_axis_th3"])
def test_wrappers_refuse_malformed_input_without_a_device(name):
    """Pure host checks: every malformed input is a ValueError before any library call; well-formed input gets past them (to the
    missing device).  The library makes the same checks itself (PGORB_E_ARG): test_gpu_library_refuses_malformed_input."""
    c = single(name)
    with pytest.raises(AttributeError):
        _wrapper_call(c)
    for what, over in _bad_inputs(c):
        with pytest.raises(ValueError):
            _wrapper_call(c, **over)
            pytest.fail(what)


def test_null_context_is_an_argument_error():
    from pilotguru_amd import _lib
    L = _lib.lib()
    z = np.zeros(64, np.float32)
    p = C.c_void_p(z.ctypes.data)
    b = (0.0, 1.0, 0.0, 1.0)
    assert L.pgorb_search_local_points(None, p, p, 0, *b, p, None, 0, p, p, None, None, 0, p, None, 0.5, 1.0, 0.8, *([p] * 8)) == _lib.PGORB_E_ARG
    assert L.pgorb_search_by_projection_last_frame(None, p, p, 0, *b, p, None, p, 0, p, None, 0, p, p, None, 1.0, 1, p, p, p, p) == _lib.PGORB_E_ARG
    assert L.pgorb_search_by_projection_keyframe_pose(None, p, p, 0, *b, p, None, p, 0, p, None, 0, p, p, None, 1.0, 100, 1, p, p, p, p) == _lib.PGORB_E_ARG
    assert L.pgorb_search_local_points_batch_device(None, p, p, p, 1, p, p, None, 0, *b, p, None, 0, p, p, None, None, 1, p, p, None, 0.5, 1.0, 0.8,
                                                    *([p] * 9), None) == _lib.PGORB_E_ARG


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(1000, 1.2, TC.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=4)
    assert np.array_equal(e.GetScaleFactors(), SF)
    yield e
    e.close()


def _check(c, got, what):
    d = TC.differences(c.kind, want(c), got)
    assert not d, "%s (%s): %s differ from the reference" % (c.name, what, d)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SINGLE_NAMES)
def test_gpu_single_call_batch_and_existing_matcher_equal_the_reference(ext, name):
    c = single(name)
    w = want(c)
    _check(c, TC.run_gpu(c, ext), "single call")
    one = TC.run_gpu_batch(TC.as_batch(c), ext)[0]
    _check(c, one, "one-pair batch")                                  # ... so the single call equals pair 0 of a one-pair batch
    nm, asg = TC.run_existing(c, ext, w["front"])
    assert nm == w["nmatches"] and np.array_equal(asg, w["assigned"]), "%s: the existing matcher on the reference's front part" % name


@pytest.mark.gpu
@pytest.mark.parametrize("kind", BATCH_KINDS)
def test_gpu_batch_equals_the_reference_on_any_stream_and_twice(ext, kind):
    import torch
    b = batch(kind)
    res, raw = TC.run_gpu_batch(b, ext, raw=True)
    for (_, _, c), r in zip(b.pairs, res):
        _check(c, r, "batched")
    again = TC.run_gpu_batch(b, ext, raw=True)[1]
    other = TC.run_gpu_batch(b, ext, stream=torch.cuda.Stream(), raw=True)[1]
    assert again == raw, "a repeated call on the same context gives other bytes"
    assert other == raw, "a second stream gives other bytes"


def _library_call(ext, c, th=None, bounds=None, idx=None, slots=None):
    """The single call straight through ctypes (no wrapper checks)."""
    L, h = ext._L, ext._h
    keep = []
    p = lambda a: C.c_void_p(a.ctypes.data)

    def opt(a):
        if a is None:
            return None
        keep.append(np.ascontiguousarray(a, np.uint8))
        return p(keep[-1])
    pts, pd, bad, obs = TC.table_arrays(c.points)
    P = np.ascontiguousarray(c.pose, TC.KF_POSE_DTYPE).reshape(())
    n = len(c.keys)
    k, d = np.ascontiguousarray(c.keys), np.ascontiguousarray(c.desc)
    b = TC.BOUNDS if bounds is None else bounds
    th = c.th if th is None else th
    out = np.zeros(max(n, 1), np.int32)
    if c.kind == "local":
        q = np.ascontiguousarray(c.queries if idx is None else idx, np.int32)
        sl = np.ascontiguousarray(c.slots if slots is None else slots, np.int32)
        o = [np.zeros(len(q), dt) for dt in (np.uint8, np.float32, np.float32, np.int32, np.float32)]
        return L.pgorb_search_local_points(h, p(k), p(d), n, *b, p(P), p(sl), len(pts), p(pts), p(pd), p(bad), p(obs), len(q), p(q), opt(c.query_seen),
                                           0.5, th, 0.8, *[p(x) for x in o], None, None, p(out))
    op = np.ascontiguousarray(c.other_point if idx is None else idx, np.int32)
    ok = np.ascontiguousarray(c.other_keys)
    flag, has = opt(c.flag), opt(c.has)
    if c.kind == "last":
        return L.pgorb_search_by_projection_last_frame(h, p(k), p(d), n, *b, p(P), has, p(ok), len(op), p(op), flag, len(pts), p(pts), p(pd),
                                                       p(obs), th, int(c.ori), None, None, None, p(out))
    return L.pgorb_search_by_projection_keyframe_pose(h, p(k), p(d), n, *b, p(P), has, p(ok), len(op), p(op), flag, len(pts), p(pts), p(pd),
                                                      p(bad), th, c.orb_dist, int(c.ori), None, None, None, p(out))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["local_th5", "last_axis_no_ori", "kf_axis_th3"])
def test_gpu_library_refuses_malformed_input(ext, name):
    from pilotguru_amd import _lib
    c = single(name)
    assert _library_call(ext, c) == want(c)["nmatches"]
    for what, over in _bad_inputs(c):
        assert _library_call(ext, c, **over) == _lib.PGORB_E_ARG, what
