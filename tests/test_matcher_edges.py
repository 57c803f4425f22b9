"""Constructed edge cases of the Frame grid and the guided matchers (tests/matcher_cases.py), checked against an independent
plain reference (tests/matcher_reference.py) as well as the oracle (oracle/match_oracle.c).

Each family asserts that the reference saw its target edge (a hit count > 0); the mutation test shows that every wrong
reading of a rule (matcher_reference.MUTANTS) changes the result of at least one case.  On the GPU the single-call ABI
and the batched device forms (h) run every case; pgorb_undistort_keypoints_batch_device (i) is checked on its own."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matcher_reference as R  # noqa: E402
from matcher_cases import (BOUNDS, FAMILIES, H, NLEVELS, SCALE, SF, TARGETS, W, _batch_groups, _case_frames, _family_ids,  # noqa: E402
                           _log_sf, all_cases, f32, grid_groups, run_gpu, run_gpu_batched, run_gpu_grid_batched, run_oracle,
                           run_reference, same)
from pilotguru_amd.orb import KEYPOINT_DTYPE  # noqa: E402

# ---------------------------------------------------------------- CPU: reference == oracle, hit counts, mutants
@pytest.mark.parametrize("family", _family_ids())
def test_reference_equals_oracle_on_constructed_family(oracle, family):
    assert np.array_equal(SF, oracle.OrbOracle(1000, SCALE, NLEVELS, 20, 7).scale_factors)
    hits = collections.Counter()
    cases = FAMILIES[family](np.random.RandomState(ord(family)))
    assert cases
    for case in cases:
        want = run_reference(case, hits=hits)
        got = run_oracle(case, oracle)
        assert same(want, got), "%s: reference %r != oracle %r" % (case["name"], want, got)
    missed = [t for t in TARGETS[family] if hits[t] == 0]
    assert not missed, "family %s never reached %s (hits %s)" % (family, missed, dict(hits))


def test_constructed_cases_reach_matches_and_rejections():
    """The cases are not vacuous: every matcher form produces matches in some cases and rejections in others."""
    made, empty = collections.Counter(), collections.Counter()
    for case in all_cases(1):
        if case["kind"] in ("grid", "area"):
            continue
        res = run_reference(case)
        (made if res[0] > 0 else empty)[case["kind"]] += 1
    for kind in ("sfi", "points", "frame", "keyframe", "bow"):
        assert made[kind] > 0 and empty[kind] > 0, (kind, made, empty)


def test_every_rule_mutant_is_caught():
    cases = all_cases(2)
    want = [run_reference(c) for c in cases]
    for name, rules in R.MUTANTS.items():
        caught = [c["name"] for c, w in zip(cases, want) if not same(run_reference(c, rules), w)]
        assert caught, "mutant %s agrees with the reference on every constructed case" % name


def test_reference_equals_oracle_on_synthetic_rides(oracle):
    """The existing synthetic frame pairs of test_frame_matcher.py: the reference agrees with the oracle there too."""
    from test_frame_matcher import _frames, _keyframe_queries, _synthetic_map_points
    ride, fr = _frames(oracle, nf=600)
    (k1, d1), (k2, d2) = fr
    bounds = BOUNDS
    start, idx = oracle.frame_grid(k2, bounds)
    rs, ri = R.Grid(k2, bounds).csr()
    assert np.array_equal(start, rs) and np.array_equal(idx, ri)
    prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
    for win, ratio, ori in ((100, 0.9, True), (30, 0.7, False)):
        want = R.search_for_initialization(k1, d1, k2, d2, bounds, prev, win, ratio, ori)
        assert same(want, oracle.search_for_initialization(k1, d1, k2, d2, bounds, prev, win, ratio, ori)) and want[0] > 50
    rng = np.random.RandomState(3)
    sel, valid, px, py, lvl, vc, pd, obs = _synthetic_map_points(k1, d1, (7, 3), rng)
    has = (rng.uniform(size=len(k2)) > 0.9).astype(np.uint8)
    for th, ratio in ((3.0, 0.8), (1.0, 0.6)):
        want = R.search_by_projection_points(k2, d2, bounds, SF, has, valid, px, py, lvl, vc, pd, obs, th, ratio)
        assert same(want, oracle.search_by_projection_points(k2, d2, bounds, SF, has, valid, px, py, lvl, vc, pd, obs, th, ratio)) and want[0] > 50
    ang = k1["angle"][sel].copy()
    ang[::7] = (ang[::7] + 100.0) % 360.0
    for th, ori in ((15.0, True), (7.0, False)):
        want = R.search_by_projection_frame(k2, d2, bounds, SF, None, valid, px, py, lvl, ang, pd, obs, th, ori)
        assert same(want, oracle.search_by_projection_frame(k2, d2, bounds, SF, None, valid, px, py, lvl, ang, pd, obs, th, ori)) and want[0] > 50
    KQ = _keyframe_queries(k1, d1, (7, 3), rng, SF, NLEVELS, W, H)
    _, kv, kf, ku, kvv, kd3, kmin, kmax, kang, kpd = KQ
    lf = _log_sf()
    for th, orbdist in ((10.0, 100), (3.0, 64)):
        want = R.search_by_projection_keyframe(k2, d2, bounds, SF, has, kv, kf, ku, kvv, kd3, kmin, kmax, lf, kang, kpd, th, orbdist, True)
        got = oracle.search_by_projection_keyframe(k2, d2, bounds, SF, has, kv, kf, ku, kvv, kd3, kmin, kmax, lf, kang, kpd, th, orbdist, True)
        assert same(want, got) and want[0] > 20


def test_reference_predict_scale_uses_the_log_contract(oracle):
    lf = _log_sf()
    assert lf == f32(oracle.log_f(SF[1]))
    log_f = R.contract_log_f()
    rng = np.random.RandomState(4)
    for maxd, dist in list(zip(rng.uniform(0.1, 50, 300), rng.uniform(0.1, 50, 300))) + [(10.0, 10.0), (12.0, 10.0), (1000.0, 1.0), (0.0, 1.0), (1.0, 0.0)]:
        assert R.predict_scale(maxd, dist, lf, NLEVELS, log_f) == oracle.predict_scale(maxd, dist, lf, NLEVELS)


def test_c_round_and_three_maxima_by_hand():
    """Spot values of the two helpers every histogram depends on, stated from the upstream text."""
    assert [R.c_round(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 0.49999997)] == [1, 2, 3, -1, -2, 0]
    assert R.compute_three_maxima([10, 0, 1] + [0] * 27) == (0, 2, -1)           # 1 < 0.1f*10 is false
    assert R.compute_three_maxima([21, 2] + [0] * 28) == (0, -1, -1)
    assert R.compute_three_maxima([30, 3] + [0] * 28) == (0, 1, -1)               # 0.1f*30 rounds to 3.0f
    assert R.compute_three_maxima([5, 5, 5, 5] + [0] * 26) == (0, 1, 2)           # count ties go to the earlier bin
    assert R.compute_three_maxima([0] * 30) == (-1, -1, -1)
    assert R.rotation_bin(10.0, 10.0) == 0 and R.rotation_bin(10.0, 10.0001) == 12 and R.rotation_bin(15.0, 0.0) == 1


class _HostFrame:
    """A frame without a device (ext is None): the wrappers' own checks come before any library call."""

    def __init__(self, n, ndesc=None):
        self.ext, self.N, self.bounds = None, n, BOUNDS
        self.mvKeys = self.mvKeysUndistorted = np.zeros(n, KEYPOINT_DTYPE)
        self.mDescriptors = np.zeros((n if ndesc is None else ndesc, 32), np.uint8)


def _wrapper_calls():
    """(call, well-formed arguments, [(name, arguments that must be refused)]) for every matcher wrapper; N = 4, 3 queries."""
    import pilotguru_amd as pg
    m, n, q = pg.ORBmatcher(), 4, 3
    F, Fshort = _HostFrame(n), _HostFrame(n, n - 1)
    u8, f4, i4 = (lambda k: np.ones(k, np.uint8)), (lambda k: np.zeros(k, np.float32)), (lambda k: np.zeros(k, np.int32))
    d32 = lambda k: np.zeros((k, 32), np.uint8)
    fv = (np.array([1, 2], np.uint32), np.array([0, 2, 4], np.int32), np.arange(4, dtype=np.uint32))
    bad_fv = [("FeatureVector starts of the wrong length", (fv[0], fv[1][:2], fv[2])),
              ("FeatureVector features shorter than start[nfv]", (fv[0], fv[1], fv[2][:3]))]
    masks = [("short kp_has_point", dict(kp_has_point=u8(n - 1))), ("long kp_has_point", dict(kp_has_point=u8(n + 1))),
             ("frame descriptors short", dict(F=Fshort))]
    pts = dict(F=F, kp_has_point=u8(n), valid=u8(q), proj_x=f4(q), proj_y=f4(q), level=i4(q), view_cos=f4(q), descriptors=d32(q),
               has_obs=u8(q))
    last = dict(F=F, kp_has_point=None, valid=u8(q), u=f4(q), v=f4(q), last_octave=i4(q), last_angle=f4(q), point_desc=d32(q),
                point_has_obs=u8(q))
    kf = dict(F=F, kp_has_point=None, valid=u8(q), already_found=u8(q), u=f4(q), v=f4(q), dist3d=f4(q), min_distance=f4(q),
              max_distance=f4(q), kf_angle=f4(q), point_desc=d32(q))
    bow = dict(F=F, kf_desc=d32(n), kf_angle=f4(n), kf_point_valid=u8(n), kf_featvec=fv, f_featvec=fv)
    sfi = dict(F1=F, F2=_HostFrame(n + 1), vbPrevMatched=np.zeros((n, 2), np.float32))
    return {
        "points": (lambda F, kp_has_point, **a: m.SearchByProjection(F, pg.MapPoints(**a), 3.0, kp_has_point), pts,
                   masks + [("short proj_x", dict(proj_x=f4(q - 1))), ("long level", dict(level=i4(q + 1))),
                            ("short query descriptors", dict(descriptors=d32(q - 1))), ("short has_obs", dict(has_obs=u8(q - 1)))]),
        "last_frame": (lambda F, kp_has_point, **a: m.SearchByProjectionLastFrame(F, th=7.0, kp_has_point=kp_has_point, **a), last,
                       masks + [("short u", dict(u=f4(q - 1))), ("long last_angle", dict(last_angle=f4(q + 1))),
                                ("short point_desc", dict(point_desc=d32(q - 1))), ("short point_has_obs", dict(point_has_obs=u8(q - 1)))]),
        "keyframe": (lambda F, kp_has_point, **a: m.SearchByProjectionKeyFrame(F, th=7.0, ORBdist=100, kp_has_point=kp_has_point, **a), kf,
                     masks + [("short already_found", dict(already_found=u8(q - 1))), ("long dist3d", dict(dist3d=f4(q + 1))),
                              ("short max_distance", dict(max_distance=f4(q - 1))), ("short kf_angle", dict(kf_angle=f4(q - 1))),
                              ("long point_desc", dict(point_desc=d32(q + 1)))]),
        "bow": (lambda **a: m.SearchByBoW(None, **a), bow,
                [("short kf_point_valid", dict(kf_point_valid=u8(n - 1))), ("short kf_desc", dict(kf_desc=d32(n - 1))),
                 ("long kf_desc", dict(kf_desc=d32(n + 1))), ("frame descriptors short", dict(F=Fshort))] +
                [(k, dict(kf_featvec=v)) for k, v in bad_fv] + [(k, dict(f_featvec=v)) for k, v in bad_fv]),
        "sfi": (lambda **a: m.SearchForInitialization(**a), sfi,
                [("short vbPrevMatched", dict(vbPrevMatched=np.zeros((n - 1, 2), np.float32))),
                 ("flat vbPrevMatched", dict(vbPrevMatched=np.zeros(2 * n, np.float32))),
                 ("vbPrevMatched of 3 columns", dict(vbPrevMatched=np.zeros((n, 3), np.float32))),
                 ("F1 descriptors short", dict(F1=Fshort)), ("F2 descriptors short", dict(F2=_HostFrame(n + 1, n)))]),
    }


@pytest.mark.parametrize("form", ["points", "last_frame", "keyframe", "bow", "sfi"])
def test_python_wrapper_rejects_short_masks_and_inconsistent_feature_vectors(form):
    """The wrappers hand the library one count per frame and per query set and every array by pointer: a per-query array,
    mask or descriptor block of another length, a vbPrevMatched that is not (N1, 2) and a FeatureVector whose arrays disagree
    are refused with ValueError before any library call.  Well-formed input gets past the checks (to the missing device)."""
    call, good, bad = _wrapper_calls()[form]
    with pytest.raises(AttributeError):
        call(**good)
    for name, kw in bad:
        with pytest.raises(ValueError):
            call(**dict(good, **kw))
            pytest.fail(name)


@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(1000, SCALE, NLEVELS, 20, 7, max_width=W, max_height=H, max_batch=4)
    assert np.array_equal(e.GetScaleFactors(), SF)
    assert f32(e.log_scale_factor()) == _log_sf()
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", _family_ids())
def test_gpu_single_calls_and_batched_forms_equal_the_reference(oracle, ext, family):
    cases = FAMILIES[family](np.random.RandomState(ord(family)))
    for case in cases:
        want = run_reference(case)
        if case["kind"] != "area":
            got = run_gpu(case, ext)
            assert same(want, got), "%s: reference %r != single call %r" % (case["name"], want, got)
    for gi_, group in enumerate(_batch_groups(cases)):
        grids, res = run_gpu_batched(group, ext, "nan" if gi_ % 2 == 0 else "huge")
        frames = [fb for c in group for fb in _case_frames(c)]
        if group[0]["kind"] in ("sfi", "bow"):                            # first frames of every pair, then second frames
            frames = [_case_frames(c)[0] for c in group] + [_case_frames(c)[1] for c in group]
        for (k, b), g in zip(frames, grids):
            assert same(R.Grid(k, b).csr(), g), "batched grid in group of %s" % group[0]["name"]
        for c, r in zip(group, res):
            assert same(run_reference(c), r), "%s: batched form %r" % (c["name"], r)
    for gi_, group in enumerate(grid_groups(cases)):                      # the grid cases through the batched grid as well
        for c, g in zip(group, run_gpu_grid_batched(group, ext, "huge" if gi_ % 2 == 0 else "nan")):
            assert same(run_reference(c), g), "%s: batched grid %r" % (c["name"], g)


@pytest.mark.gpu
def test_gpu_search_by_bow_refuses_feature_vectors_outside_the_frame(ext):
    """pgorb_search_by_bow checks both FeatureVectors as pgorb_search_for_triangulation does: a feature index >= n, a first
    start other than 0 or a descending start is PGORB_E_ARG (the kernel would read outside the frame's slot).  An empty side
    still gives all -1 and 0, with NULL FeatureVector pointers allowed when nfv == 0."""
    import pilotguru_amd as pg
    from matcher_cases import ArrayFrame, keys, rand_desc
    from pilotguru_amd import _lib
    rng = np.random.RandomState(11)
    n = 4
    k = keys([100.0, 200.0, 300.0, 400.0], [100.0, 150.0, 200.0, 250.0])
    kd, F = rand_desc(rng, n), ArrayFrame(ext, k, rand_desc(rng, n), BOUNDS)
    ka, kv = k["angle"].copy(), np.ones(n, np.uint8)
    m = pg.ORBmatcher(0.9, True)
    fv = (np.array([1, 2], np.uint32), np.array([0, 2, 4], np.int32), np.arange(4, dtype=np.uint32))
    nm, mt = m.SearchByBoW(ext, kd, ka, kv, fv, F, fv)
    assert nm >= 0 and len(mt) == n
    bad = [(fv[0], fv[1], np.array([0, 1, 2, 4], np.uint32)), (fv[0], np.array([1, 2, 4], np.int32), fv[2]),
           (fv[0], np.array([0, 3, 2], np.int32), fv[2])]
    for b in bad:
        for kfv, ffv in ((b, fv), (fv, b)):
            with pytest.raises(_lib.PgorbError) as e:
                m.SearchByBoW(ext, kd, ka, kv, kfv, F, ffv)
            assert e.value.code == _lib.PGORB_E_ARG
    empty = (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32))
    for kfv, ffv in ((empty, fv), (fv, empty)):
        nm, got = m.SearchByBoW(ext, kd, ka, kv, kfv, F, ffv)
        assert nm == 0 and (got == -1).all()
    nm, got = m.SearchByBoW(ext, np.zeros((0, 32), np.uint8), np.zeros(0, np.float32), np.zeros(0, np.uint8), empty, F, fv)
    assert nm == 0 and (got == -1).all()
    p = lambda a: C.c_void_p(a.ctypes.data)
    out = np.full(n, 7, np.int32)
    fa = F.mvKeys["angle"].copy()
    assert ext._L.pgorb_search_by_bow(ext._h, p(kd), p(ka), p(kv), n, None, None, None, 0, p(F.mDescriptors), p(fa), n,
                                      p(fv[0]), p(fv[1]), p(fv[2]), 2, C.c_float(0.9), 1, p(out)) == 0
    assert (out == -1).all()


@pytest.mark.gpu
def test_gpu_undistort_keypoints_batch_device(oracle, ext):
    """pgorb_undistort_keypoints_batch_device on a ragged batch: frame by frame bit-equal to pgorb_undistort_keypoints;
    the kernel writes slots i < min(n[f], cap) only (k_undistort_keypoints), so slots past n keep what d_out held and a
    count above cap is clamped; k1 == 0 copies; a float64 forward distortion of the result reproduces the input."""
    import torch
    L, h = ext._L, ext._h
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cam = np.array([700.0, 690.0, 322.5, 238.25], np.float32)
    rng = np.random.RandomState(12)
    ns = [37, 0, 64, 1, 70]                                     # the last count exceeds cap: clamped
    cap = 64
    kp = np.zeros((len(ns), cap), KEYPOINT_DTYPE)
    kp["x"] = rng.uniform(-20, 660, kp.shape); kp["y"] = rng.uniform(-20, 500, kp.shape)
    kp["angle"] = rng.uniform(0, 360, kp.shape); kp["octave"] = rng.randint(0, 8, kp.shape); kp["size"] = 31.0; kp["response"] = 0.5
    for f, n in enumerate(ns):
        kp[f, n:]["x"], kp[f, n:]["y"] = np.nan, 3.0e38                # poisoned slots past n
    din = torch.from_numpy(kp.view(np.uint8).reshape(len(ns), cap, 28).copy()).cuda()
    dn = torch.tensor(ns, dtype=torch.int32, device="cuda")
    sentinel = np.uint8(0xA5)
    for dist in ([-0.25, 0.08, 0.001, -0.0007, 0.0], [0.12, -0.3, -0.002, 0.0015, 0.05], [0.0, 0.08, 0.001, -0.0007, 0.0]):
        dc = np.array(dist, np.float32)
        dout = torch.full((len(ns), cap, 28), int(sentinel), dtype=torch.uint8, device="cuda")
        ext._check(L.pgorb_undistort_keypoints_batch_device(h, p(din), p(dn), len(ns), cap, C.c_void_p(cam.ctypes.data),
                                                           C.c_void_p(dc.ctypes.data), p(dout), s))
        torch.cuda.synchronize()
        out = dout.cpu().numpy()
        for f, n in enumerate(ns):
            m = min(n, cap)
            got = out[f, :m].copy().view(KEYPOINT_DTYPE).reshape(-1)
            single = np.zeros(m, KEYPOINT_DTYPE)
            if m:
                src = np.ascontiguousarray(kp[f, :m])
                ext._check(L.pgorb_undistort_keypoints(h, C.c_void_p(src.ctypes.data), m, C.c_void_p(cam.ctypes.data),
                                                       C.c_void_p(dc.ctypes.data), C.c_void_p(single.ctypes.data)))
            assert got.tobytes() == single.tobytes(), "frame %d" % f
            assert got.tobytes() == oracle.undistort_keypoints(kp[f, :m], cam, dc).tobytes()
            assert np.all(out[f, m:] == sentinel), "frame %d: a slot past n was written" % f
            for fld in ("size", "angle", "response", "octave", "class_id"):
                assert got[fld].tobytes() == kp[f, :m][fld].tobytes()
            if dist[0] == 0.0:
                assert got.tobytes() == kp[f, :m].tobytes()          # Frame.cc:410-414: the keypoints as they are
            elif m:
                fx, fy, cx, cy = (float(v) for v in cam)
                k1, k2, p1, p2, k3 = (float(v) for v in dc)
                x = (got["x"].astype(np.float64) - cx) / fx; y = (got["y"].astype(np.float64) - cy) / fy
                r2 = x * x + y * y
                cd = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
                xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
                yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
                res = np.maximum(np.abs(xd * fx + cx - kp[f, :m]["x"]), np.abs(yd * fy + cy - kp[f, :m]["y"]))
                assert res.max() < 0.05, (f, dist, res.max())
