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
