"""pgorb_pose_optimization (pilotguru_amd/csrc/pose_opt.hip): Optimizer::PoseOptimization on the device, against the plain
reference of tests/pose_reference.py on the problems of tests/pose_cases.py.

The reference is UNPINNED to g2o (it cannot be built where the suite runs); the CPU tests below anchor it: its Jacobian against
central differences of its own error under its own exp(update) * estimate, its 6 x 6 solve against numpy.linalg.solve, and
noise-free scenes that return the generating pose with every edge an inlier.

Tolerances.  Integers and flags are compared exactly, the pose of an untouched problem as bytes.  The float outputs get, per
case and output, the larger of 2 float ulps at the output's scale and 16 x the spread the reference shows between its three
summation orders (tests/golden/pose_opt_spread.json, written by tests/golden/make_pose_opt_spread.py): pose_cases.bounds.  The
iteration and trial counts are reported, not compared."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_cases as PC  # noqa: E402
import pose_reference as PR  # noqa: E402

f32, f64 = np.float32, np.float64
CASE_NAMES = ["few_0", "few_2", "few_3", "nine", "ten", "clean_64", "clean_65", "clean_257", "outliers_300", "reclassified",
              "all_outliers_after_round0", "lm_rejected", "small_angle", "far_translation", "sparse_2000", "z_zero", "no_obs_points",
              "cap_16000", "huber_rounds"]
BATCH_NAMES = ["batch_0_edges", "batch_2_edges", "batch_65_edges", "batch_300_edges", "batch_cap_edges", "batch_frame_repeat"]
NEW_SYMBOLS = ["pgorb_pose_optimization", "pgorb_pose_optimization_batch_device", "pgorb_slots_from_assignment",
               "pgorb_slots_from_assignment_batch_device"]
_cache = {}


def cases():
    if "cases" not in _cache:
        _cache["cases"] = {c.name: c for c in PC.single_cases()}
        _cache["batch"] = PC.batch()
        _cache["cases"].update({c.name: c for _, c in _cache["batch"].pairs})
    return _cache["cases"]


def batch():
    cases()
    return _cache["batch"]


def want(name, discard=False):
    """The reference's result, computed once and shared (with the round-by-round trace and the hit counters)."""
    key = ("want", name, discard)
    if key not in _cache:
        hits, trace = {}, []
        _cache[key] = (PC.run_reference(cases()[name], hits=hits, discard=discard, trace=trace), hits, trace)
    return _cache[key][0]


def recorded():
    if "spread" not in _cache:
        with open(os.path.join(HERE, "golden", "pose_opt_spread.json")) as f:
            _cache["spread"] = json.load(f)
    return _cache["spread"]


# ---------------------------------------------------------------- CPU
def test_symbols_and_mirror_exist():
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(HERE), "include", "pgorb.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in _lib.SYMBOLS and (s + "(") in header
    assert callable(pg.Optimizer.PoseOptimization)
    assert (pg.PO_FEW, pg.PO_NONFINITE, pg.PO_INFO) == (PR.PO_FEW, PR.PO_NONFINITE, 8)


def test_case_list_is_what_the_tests_name():
    assert [c.name for c in PC.single_cases()] == CASE_NAMES == PC.CASE_NAMES
    b = batch()
    assert [c.name for _, c in b.pairs] == BATCH_NAMES
    assert [c.edges for _, c in b.pairs] == [0, 2, 65, 300, b.cap, 300] and b.cap % 64 != 0
    assert [f for f, _ in b.pairs] == [2, 2, 2, 1, 0, 1] and len(b.frames) == 3
    c = cases()
    assert (c["few_0"].edges, c["few_2"].edges, c["few_3"].edges, c["nine"].edges, c["ten"].edges) == (0, 2, 3, 9, 10)
    assert (c["clean_64"].edges, c["clean_65"].edges, c["clean_257"].edges, c["outliers_300"].edges) == (64, 65, 257, 300)
    assert (c["sparse_2000"].n, c["sparse_2000"].edges) == (2000, 150)
    assert c["cap_16000"].n == c["cap_16000"].edges == PC.MAX_N
    assert abs(float(np.abs(c["far_translation"].pose["Tcw"].reshape(3, 4)[:, 3]).max()) - 64.0) < 3.0      # |t| about 100


def test_every_hit_the_cases_are_built_for_is_counted():
    for name, hit in PC.CASE_HITS.items():
        want(name)
        assert _cache[("want", name, False)][1].get(hit, 0) > 0, "%s never reaches '%s'" % (name, hit)
    w = want
    assert w("few_0")["status"] == w("few_2")["status"] == PR.PO_FEW and w("few_2")["ret"] == 0
    assert w("few_3")["rounds"] == w("nine")["rounds"] == 1 and w("ten")["rounds"] == 4
    assert w("z_zero")["status"] == PR.PO_NONFINITE
    assert w("no_obs_points")["nmatches_map"] < w("no_obs_points")["ret"]
    # the empty active set: the later rounds leave the input pose
    a = w("all_outliers_after_round0")
    assert a["ret"] == 0 and np.array_equal(a["Tcw"], PR.to_pose_floats(PR.to_se3(cases()["all_outliers_after_round0"].pose["Tcw"]))[0])
    # discard_outliers: the outlier slots are emptied and their flags cleared; the count is the same
    k, d = w("outliers_300"), w("outliers_300", True)
    out = k["outlier"] != 0
    assert out.sum() == 300 - k["ret"] > 0 and not d["outlier"].any() and (d["kp_point_out"][out] == -1).all()
    assert np.array_equal(d["kp_point_out"][~out], k["kp_point_out"][~out]) and d["nmatches_map"] == k["nmatches_map"]


@pytest.mark.parametrize("mutant", sorted(PR.MUTANTS))
def test_every_mutant_changes_a_compared_output(mutant):
    """On at least one case (the chi2-in-double mutant: on the probe built for it, which no compared case can be -- see its
    docstring)."""
    rules = PR.MUTANTS[mutant]
    names = [n for n in CASE_NAMES + BATCH_NAMES if n != "cap_16000"]
    for n in names:
        if PC.differences(cases()[n], want(n), PC.run_reference(cases()[n], rules=rules), recorded()[n]):
            return
    if mutant == "chi2_in_double":
        c = PC.chi2_window_probe()
        tr = []
        w = PC.run_reference(c, trace=tr)
        v = tr[0][1][5]
        assert v > f64(f32(5.991)) and f32(v) == f32(5.991), "the probe's chi2 left the window"
        assert PC.differences(c, w, PC.run_reference(c, rules=rules), dict.fromkeys(PC.FLOAT_OUTPUTS, 0.0))
        return
    pytest.fail("no case notices the mutant %s" % mutant)


def test_anchor_jacobian_equals_central_differences():
    """... of the reference's own error under its own exp(update) * estimate: the signs, the column order (omega, upsilon) and the
    update side."""
    rng = np.random.RandomState(3)
    for _ in range(20):
        P = PC.true_pose(rng)
        X, uv, _ = PC.observe(rng, PC.se3_matrix(P), 5, 2.0)
        E = PR.Edges(X, uv, np.ones(5, f32), np.arange(5), (PC.FX, PC.FX, PC.CX, PC.CY))
        pc, _, _ = PR.edge_error(P, E)
        J0, J1 = PR.jacobian(pc, E.cam)
        h = 1e-6
        for d in range(6):
            u = np.zeros(6)
            u[d] = h
            _, a0, a1 = PR.edge_error(PR.oplus(P, u), E)
            _, b0, b1 = PR.edge_error(PR.oplus(P, -u), E)
            assert np.allclose((a0 - b0) / (2 * h), J0[d], rtol=1e-6, atol=1e-4), d
            assert np.allclose((a1 - b1) / (2 * h), J1[d], rtol=1e-6, atol=1e-4), d


def test_anchor_solve_agrees_with_numpy():
    rng = np.random.RandomState(4)
    for _ in range(50):
        A = rng.normal(0, 1, (9, 6))
        H = A.T @ A + np.eye(6) * rng.uniform(1e-3, 1.0)
        b = rng.normal(0, 1, 6)
        x, ok = PR.ldlt_solve(H, b)
        assert ok and np.allclose(x, np.linalg.solve(H, b), rtol=1e-9, atol=1e-12)
    assert not PR.ldlt_solve(-np.eye(6), np.ones(6))[1]


@pytest.mark.parametrize("name", ["few_3", "nine", "ten", "clean_64", "clean_65", "clean_257", "lm_rejected", "small_angle", "far_translation"])
def test_anchor_noise_free_scenes_return_the_generating_pose(name):
    """To float rounding: the points and observations are floats, so the minimum sits within a few float ulps of the generating pose."""
    c, w = cases()[name], want(name)
    T = PC.se3_matrix(c.true)
    assert w["ret"] == c.edges and not w["outlier"].any()
    d = PC.scaled_differences(dict(Tcw=T.astype(f32).reshape(12), Ow=np.zeros(3), chi2=[]), dict(Tcw=w["Tcw"], Ow=np.zeros(3), chi2=[]))
    assert d["R"] < 4e-7 and d["t"] < (4e-6 if name == "few_3" else 1e-6), d


def test_spread_file_is_up_to_date_with_the_cases():
    rec = recorded()
    assert sorted(rec) == sorted(CASE_NAMES + BATCH_NAMES)
    for n in CASE_NAMES + BATCH_NAMES:
        got = PC.spread(cases()[n])
        assert got == {k: rec[n][k] for k in PC.FLOAT_OUTPUTS}, "%s: run tests/golden/make_pose_opt_spread.py" % n


@pytest.mark.parametrize("name", CASE_NAMES + BATCH_NAMES)
def test_case_condition(name):
    """Under all three summation orders the reference gives identical outlier flags after every round, and every chi2 at every
    classification is further than 1e-4 (relative) from 5.991."""
    traces = []
    for order in PR.ORDERS:
        tr = []
        PC.run_reference(cases()[name], order, trace=tr)
        traces.append(tr)
    for tr in traces:
        assert len(tr) == len(traces[0])
        for (fl, c2), (fl0, _) in zip(tr, traces[0]):
            assert np.array_equal(fl, fl0), "%s: the flags depend on the summation order" % name
            assert (np.abs(c2 / 5.991 - 1.0) > 1e-4).all(), "%s: a chi2 within 1e-4 of the threshold" % name


class _HostFrame:
    """A frame without a device (ext is None): the mirror's own checks come before any library call."""

    def __init__(self, c, keys=None):
        self.ext, self.N = None, c.n
        self.mvKeysUndistorted = PC.keypoints(c.keys_xy, c.octaves) if keys is None else keys


def _table(c, points=None):
    import pilotguru_amd as pg
    pts = PC.table(c.points if points is None else points)
    n = len(pts)
    return pg.MapPointTable(pts, np.zeros((n, 32), np.uint8), None, np.arange(n + 1, dtype=np.int32), np.zeros(max(n, 1), np.uint64))


def _bad_inputs(c):
    """(name, what to change) every checked call must refuse: see include/pgorb.h."""
    held = np.flatnonzero(c.kp_point >= 0)
    hi, lo = c.kp_point.copy(), c.kp_point.copy()
    hi[0], lo[1] = len(c.points), -2
    bad = [("index == npoints", dict(kp_point=hi)), ("index < -1", dict(kp_point=lo))]
    for k, v in (("Tcw", np.nan), ("Tcw", np.inf), ("fx", np.nan), ("cy", np.inf), ("fx", 0.0), ("fy", 0.0)):
        P = PC.pose_record(c.pose).copy()
        if k == "Tcw":
            P["Tcw"][7] = v
        else:
            P[k] = v
        bad.append(("%s = %r" % (k, v), dict(pose=P)))
    pts = c.points.copy()
    pts[c.kp_point[held[2]], 1] = np.nan
    bad.append(("a referenced point is NaN", dict(points=pts)))
    return bad


def _mirror_call(c, F=None, **over):
    import pilotguru_amd as pg
    return pg.Optimizer.PoseOptimization(_HostFrame(c) if F is None else F, over.get("pose", PC.pose_record(c.pose)), over.get("kp_point", c.kp_point),
                                         _table(c, over.get("points")), False)


def test_mirror_refuses_malformed_input_without_a_device():
    """Pure host checks: every malformed input is a ValueError before any library call; well-formed input gets past them (to the
    missing device).  An unreferenced point may be anything.  The library makes the same checks itself (PGORB_E_ARG):
    test_gpu_library_and_mirrors_refuse_malformed_input."""
    c = cases()["ten"]
    with pytest.raises(AttributeError):
        _mirror_call(c)
    pts = c.points.copy()
    pts[np.setdiff1d(np.arange(len(pts)), c.kp_point)[0]] = np.nan
    with pytest.raises(AttributeError):
        _mirror_call(c, points=pts)
    for what, over in _bad_inputs(c):
        with pytest.raises(ValueError):
            _mirror_call(c, **over)
            pytest.fail(what)
    with pytest.raises(ValueError):
        _mirror_call(c, kp_point=c.kp_point[:-1])


def test_null_context_is_an_argument_error():
    from pilotguru_amd import _lib
    L = _lib.lib()
    z = np.zeros(64, np.float32)
    p = C.c_void_p(z.ctypes.data)
    assert L.pgorb_pose_optimization(None, p, 0, p, p, 0, p, None, 0, p, p, None, None, None, None) == _lib.PGORB_E_ARG
    assert L.pgorb_pose_optimization_batch_device(None, p, p, 1, None, 0, p, p, 0, p, None, 0, p, p, None, None, None, None, None, None) == _lib.PGORB_E_ARG
    assert L.pgorb_slots_from_assignment(None, p, p, 0, p, 0) == _lib.PGORB_E_ARG
    assert L.pgorb_slots_from_assignment_batch_device(None, p, p, 0, p, 1, 0, None) == _lib.PGORB_E_ARG


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(1000, 1.2, PC.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=4)
    assert np.array_equal(e.GetScaleFactors(), PC.SF)
    assert np.array_equal(np.asarray(e.GetInverseScaleSigmaSquares(), f32)[:PC.NLEVELS], PR.inv_level_sigma2())
    yield e
    e.close()


def _check(name, got, what, discard=False):
    assert not isinstance(got, int), "%s (%s): error %r" % (name, what, got)
    w = want(name, discard)
    d = PC.differences(cases()[name], w, got, recorded()[name])
    print("%s (%s): iterations %s / %s, trials %d / %d, scaled differences %s" % (
        name, what, got["iterations"], w["iterations"], got["trials"], w["trials"], PC.scaled_differences(w, got) if not w["status"] else "-"))
    assert not d, "%s (%s): %s differ from the reference" % (name, what, d)
    assert got["edges"] == w["edges"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_single_call_equals_the_reference(ext, name):
    c = cases()[name]
    got = PC.run_gpu(c, ext)
    _check(name, got, "single call")
    if want(name)["status"]:
        assert got["pose_bytes"] == np.asarray(PC.pose_record(c.pose)).tobytes(), "an untouched problem returns the input pose byte for byte"
    else:
        assert got["pose_bytes"][60:] == np.asarray(PC.pose_record(c.pose)).tobytes()[60:], "pose_out carries the input's camera fields"


@pytest.mark.gpu
def test_gpu_discard_outliers_both_ways(ext):
    c = cases()["outliers_300"]
    _check("outliers_300", PC.run_gpu(c, ext, discard=False), "kept")
    _check("outliers_300", PC.run_gpu(c, ext, discard=True), "discarded", discard=True)


def _bytes(r):
    return r["pose_bytes"] + b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("outlier", "kp_point_out", "chi2")) + \
        repr((r["ret"], r["nmatches_map"], r["status"], r["rounds"], r["iterations"], r["trials"], r["edges"])).encode()


@pytest.mark.gpu
def test_gpu_batch_equals_the_reference_and_its_singles_byte_for_byte(ext):
    """... and the determinism contract: the same bytes on a second stream, on a repeat, and for every pair when the pairs run in
    reversed order."""
    import torch
    b = batch()
    res = PC.run_gpu_batch(b, ext)
    for (f, c), r in zip(b.pairs, res):
        _check(c.name, r, "batched")
        assert r["tail_ok"], "%s: the entries past n are not the empty slots'" % c.name
        assert _bytes(PC.run_gpu(c, ext)) == _bytes(r), "%s: the single call and the batch differ" % c.name
    raw = [_bytes(r) for r in res]
    assert [_bytes(r) for r in PC.run_gpu_batch(b, ext)] == raw, "a repeated call gives other bytes"
    assert [_bytes(r) for r in PC.run_gpu_batch(b, ext, stream=torch.cuda.Stream())] == raw, "a second stream gives other bytes"
    rev = list(range(len(b.pairs)))[::-1]
    assert [_bytes(r) for r in PC.run_gpu_batch(b, ext, order=rev)][::-1] == raw, "a pair's result depends on its place in the batch"
    for discard in (True,):
        for (f, c), r in zip(b.pairs, PC.run_gpu_batch(b, ext, discard=True)):
            _check(c.name, r, "batched, discard_outliers", discard=True)


@pytest.mark.gpu
def test_gpu_slots_from_assignment_equals_its_numpy_form(ext):
    import torch
    rng = np.random.RandomState(9)
    cap, stride, npairs = 333, 77, 3
    asg = rng.randint(-1, stride, (npairs, cap)).astype(np.int32)
    asg[:, ::5] = -1
    src = rng.randint(-1, 5000, (npairs, stride)).astype(np.int32)
    kp0 = rng.randint(-1, 5000, (npairs, cap)).astype(np.int32)
    expect = np.where(asg >= 0, np.take_along_axis(src, np.maximum(asg, 0), 1), kp0)
    d = lambda a: torch.from_numpy(a.copy()).cuda()
    da, ds, dk = d(asg), d(src), d(kp0)
    p = lambda t: C.c_void_p(t.data_ptr())
    ext._check(ext._L.pgorb_slots_from_assignment_batch_device(ext._h, p(da), p(ds), stride, p(dk), cap, npairs, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(dk.cpu().numpy(), expect)
    one = kp0[0].copy()
    q = lambda a: C.c_void_p(a.ctypes.data)
    ext._check(ext._L.pgorb_slots_from_assignment(ext._h, q(asg[0]), q(src[0]), stride, q(one), cap))
    assert np.array_equal(one, expect[0])
    from pilotguru_amd import _lib
    bad = asg[0].copy()
    bad[3] = stride
    assert ext._L.pgorb_slots_from_assignment(ext._h, q(bad), q(src[0]), stride, q(one), cap) == _lib.PGORB_E_ARG


def _library_call(ext, c, n=None, **over):
    L, h = ext._L, ext._h
    n = c.n if n is None else n
    k = over.get("keys", PC.keypoints(c.keys_xy, c.octaves))
    pts = PC.table(over.get("points", c.points))
    P = np.asarray(over.get("pose", PC.pose_record(c.pose))).reshape(1).copy()
    kp = np.ascontiguousarray(over.get("kp_point", c.kp_point), np.int32)
    out, fl = np.zeros(1, P.dtype), np.zeros(max(len(kp), 1), np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    return L.pgorb_pose_optimization(h, p(k), n, p(P), p(kp), len(pts), p(pts), None, 0, p(out), p(fl), None, None, None, None)


@pytest.mark.gpu
def test_gpu_library_and_mirrors_refuse_malformed_input(ext):
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    c = cases()["ten"]
    assert _library_call(ext, c) == want("ten")["ret"]
    octs = c.octaves.copy()
    octs[np.flatnonzero(c.kp_point >= 0)[0]] = PC.NLEVELS
    bad = _bad_inputs(c) + [("an octave outside the levels", dict(keys=PC.keypoints(c.keys_xy, octs)))]
    for what, over in bad:
        assert _library_call(ext, c, **over) == _lib.PGORB_E_ARG, what
    assert _library_call(ext, c, n=-1) == _lib.PGORB_E_ARG
    # an octave outside the levels where there is no point is not read
    free = c.octaves.copy()
    free[np.flatnonzero(c.kp_point < 0)[0]] = 99
    assert _library_call(ext, c, keys=PC.keypoints(c.keys_xy, free)) == want("ten")["ret"]

    class F:
        pass
    F.ext, F.N, F.mvKeysUndistorted = ext, c.n, PC.keypoints(c.keys_xy, c.octaves)
    r = pg.Optimizer.PoseOptimization(F, PC.pose_record(c.pose), c.kp_point, _table(c))
    got = PC.result_of(r["pose"], r["outlier"], r["kp_point_out"], r["nmatches_map"], r["chi2"],
                       [r["status"], r["rounds"]] + r["iterations"] + [r["trials"], r["edges"]], r["ret"])
    _check("ten", got, "Python mirror")
    F.mvKeysUndistorted = PC.keypoints(c.keys_xy, octs)
    with pytest.raises(ValueError):
        pg.Optimizer.PoseOptimization(F, PC.pose_record(c.pose), c.kp_point, _table(c))


@pytest.mark.gpu
def test_gpu_one_past_the_keypoint_limit_is_refused(ext):
    """(The limit itself is the case cap_16000 of the single-call test.)"""
    from pilotguru_amd import _lib
    import torch
    c = cases()["cap_16000"]
    n = PC.MAX_N + 1
    k = np.zeros(n, PC.keypoints(c.keys_xy, c.octaves).dtype)
    kp = np.full(n, -1, np.int32)
    assert _library_call(ext, c, n=n, keys=k, kp_point=kp) == _lib.PGORB_E_LIMIT
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = C.c_void_p(t.data_ptr())
    assert ext._L.pgorb_pose_optimization_batch_device(ext._h, p, p, n, None, 1, p, p, 1, p, None, 0, p, p, None, None, None, None, None, None) == _lib.PGORB_E_LIMIT


# ---------------------------------------------------------------- the chain on a resident batch
def _chain_problem(c, kp_point, obs):
    """The pose problem of one pair of the chain: the pair's frame, its pose and the slots the search produced."""
    return PC.Case("chain_" + c.name, np.stack([c.keys["x"], c.keys["y"]], 1), c.keys["octave"], c.pose, kp_point,
                   np.array([p["pos"] for p in c.points], f32), obs)


def _chain_reference_front(b):
    """Per pair: the last-frame search of the reference, the slots it gives, and the pose problem they make (checked against the
    condition every compared case meets)."""
    import tracking_cases as TC
    import tracking_reference as TR
    out = []
    obs = TC.table_arrays(b.points)[3]
    for f, o, c in b.pairs:
        fr, mps = c.build()
        r1 = TR.search_by_projection_last_frame(fr, c.other_keys, [None if s < 0 else mps[s] for s in c.other_point], c.flag, c.has, c.th, c.ori)
        a = r1["assigned"]
        kp_point = np.where(a >= 0, c.other_point[np.maximum(a, 0)], -1).astype(np.int32) if len(c.other_point) else np.full(len(a), -1, np.int32)
        pc = _chain_problem(c, kp_point, obs)
        traces = []
        for order in PR.ORDERS:
            tr = []
            PC.run_reference(pc, order, discard=True, trace=tr)
            traces.append(tr)
        for tr in traces:
            for (fl, c2), (fl0, _) in zip(tr, traces[0]):
                assert np.array_equal(fl, fl0) and (np.abs(c2 / 5.991 - 1.0) > 1e-4).all(), "%s: rebuild the scene" % pc.name
        out.append((r1, kp_point, pc, PC.run_reference(pc, discard=True), PC.spread(pc)))
    return out


CHAIN_SCENES = ["pair_batch", "last_scene", "last_axis_no_ori"]


def _chain_batch(scene):
    """The four-pair last-frame batch of tests/tracking_cases.py (few edges a pair: one round, and two pairs with none), or one of
    its single last-frame scenes as a one-pair batch (four rounds; last_axis_no_ori ends with an outlier to discard)."""
    import tracking_cases as TC
    if scene == "pair_batch":
        return TC.pair_batch("last")
    return TC.as_batch([c for c in TC.single_cases() if c.name == scene][0])


def test_chain_scenes_meet_the_case_condition():
    edges, discarded = [], 0
    for scene in CHAIN_SCENES:
        for _, kp_point, pc, r3, _ in _chain_reference_front(_chain_batch(scene)):
            edges.append(pc.edges)
            discarded += int(((kp_point >= 0) & (r3["kp_point_out"] < 0)).sum())
    assert max(edges) >= 30 and min(edges) < 3 and discarded > 0


@pytest.mark.gpu
@pytest.mark.parametrize("scene", CHAIN_SCENES)
def test_gpu_chain_search_slots_pose_search_on_a_resident_batch(ext, scene):
    """pgorb_search_by_projection_last_frame_batch_device -> pgorb_slots_from_assignment_batch_device ->
    pgorb_pose_optimization_batch_device(discard_outliers = 1) -> pgorb_search_local_points_batch_device with d_pose_out and the
    discarded slots as query_seen, on the scenes of tests/tracking_cases.py and with no download in between; every stage against
    its reference (the last stage's reference reads the pose and slots the device produced, which stage three has compared)."""
    import torch
    import tracking_cases as TC
    import tracking_reference as TR
    from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE
    b = _chain_batch(scene)
    front = _chain_reference_front(b)
    L, h = ext._L, ext._h
    nf, npair, cap = len(b.frames), len(b.pairs), b.qcap
    kp = np.zeros((nf, cap), KEYPOINT_DTYPE)
    ds = np.zeros((nf, cap, 32), np.uint8)
    for f, (k, d) in enumerate(b.frames):
        kp[f, :len(k)] = k
        ds[f, :len(k)] = d
    pts, pd, bad, obs = TC.table_arrays(b.points)
    npts = len(pts)
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def rows(get, dtype, fill=0):
        x = np.full((npair, cap), fill, dtype)
        for j, (_, _, c) in enumerate(b.pairs):
            a = get(c)
            if a is not None:
                x[j, :len(a)] = a
        return dev(x)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dk, dd, dn = dev(kp.view(np.uint8).reshape(nf, cap, 28)), dev(ds), dev(np.array([len(k) for k, _ in b.frames], np.int32))
    gs = torch.empty((nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    gi = torch.empty((nf, cap), dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_frame_grid_batch_device(h, p(dk), p(dn), nf, cap, *TC.BOUNDS, p(gs), p(gi), s))
    dpts, dpd, dbad, dobs = dev(pts.view(np.uint8).reshape(npts, 32)), dev(pd), dev(bad), dev(obs)
    pose = dev(np.array([c.pose for _, _, c in b.pairs], KF_POSE_DTYPE).view(np.uint8).reshape(npair, -1))
    pf, po = dev(np.array([f for f, _, _ in b.pairs], np.int32)), dev(np.array([o for _, o, _ in b.pairs], np.int32))
    op, flag, has = rows(lambda c: c.other_point, np.int32, -1), rows(lambda c: c.flag, np.uint8), rows(lambda c: c.has, np.uint8)
    I32 = lambda *sh: torch.full(sh, -9, dtype=torch.int32, device="cuda")
    asg, nm, c0 = I32(npair, cap), I32(npair), b.pairs[0][2]
    ext._check(L.pgorb_search_by_projection_last_frame_batch_device(
        h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pf), p(po), npair, *TC.BOUNDS, p(pose), p(has), p(op), p(flag), npts, p(dpts), p(dpd), p(dobs),
        c0.th, int(c0.ori), None, None, None, p(asg), p(nm), s))
    kpp = torch.full((npair, cap), -1, dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_slots_from_assignment_batch_device(h, p(asg), p(op), cap, p(kpp), cap, npair, s))
    pose_out = torch.zeros((npair, KF_POSE_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    outl = torch.full((npair, cap), 9, dtype=torch.uint8, device="cuda")
    kpo, nmap, info, ninl = I32(npair, cap), I32(npair), I32(npair, 8), I32(npair)
    chi = torch.zeros((npair, cap), dtype=torch.float32, device="cuda")
    ext._check(L.pgorb_pose_optimization_batch_device(h, p(dk), p(dn), cap, p(pf), npair, p(pose), p(kpp), npts, p(dpts), p(dobs), 1, p(pose_out),
                                                      p(outl), p(kpo), p(nmap), p(chi), p(info), p(ninl), s))
    # the points of the discarded slots have mnLastFrameSeen = this frame's id (Tracking.cc:904): query_seen, formed on the device
    q = torch.arange(npts, dtype=torch.int32, device="cuda").repeat(npair, 1).contiguous()
    nq = torch.full((npair,), npts, dtype=torch.int32, device="cuda")
    disc = ((kpp >= 0) & (kpo < 0)).to(torch.int32)
    seen = (torch.zeros((npair, npts), dtype=torch.int32, device="cuda").scatter_add_(1, kpp.clamp(min=0).long(), disc) > 0).to(torch.uint8).contiguous()
    iv = torch.full((npair, npts), 9, dtype=torch.uint8, device="cuda")
    F32 = lambda: torch.zeros((npair, npts), dtype=torch.float32, device="cuda")
    px, py, vc, lv = F32(), F32(), F32(), I32(npair, npts)
    kpo2, ntm, asg2, nm2 = I32(npair, cap), I32(npair), I32(npair, cap), I32(npair)
    ext._check(L.pgorb_search_local_points_batch_device(
        h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pf), npair, *TC.BOUNDS, p(pose_out), p(kpo), npts, p(dpts), p(dpd), p(dbad), p(dobs), npts,
        p(nq), p(q), p(seen), 0.5, 3.0, 0.8, p(iv), p(px), p(py), p(lv), p(vc), p(kpo2), p(ntm), p(asg2), p(nm2), s))
    torch.cuda.synchronize()                                             # the first download
    H = lambda t: t.cpu().numpy()
    poses = np.frombuffer(H(pose_out).tobytes(), KF_POSE_DTYPE)
    for j, ((f, o, c), (r1, kp_point, pc, r3, spread)) in enumerate(zip(b.pairs, front)):
        n = len(c.keys)
        assert int(nm[j]) == r1["nmatches"] and np.array_equal(H(asg[j, :n]), r1["assigned"]), "%s: the search" % c.name
        assert np.array_equal(H(kpp[j, :n]), kp_point) and (H(kpp[j, n:]) == -1).all(), "%s: the slots" % c.name
        got = PC.result_of(poses[j], H(outl[j, :n]), H(kpo[j, :n]), nmap[j], H(chi[j, :n]), H(info[j]), ninl[j])
        d = PC.differences(pc, r3, got, spread)
        assert not d, "%s: the pose optimisation differs from the reference: %s" % (c.name, d)
        # the local points under the device's pose and slots
        fr, mps = c.build()
        fr = TR.Frame(1, c.keys, c.desc, TC.BOUNDS, poses[j], TC.SF, TC.log_sf(), TC.NLEVELS)
        fr.slots = [None if t < 0 else mps[t] for t in got["kp_point_out"]]
        seen_ref = np.zeros(npts, np.uint8)
        seen_ref[kp_point[(kp_point >= 0) & (got["kp_point_out"] < 0)]] = 1
        assert np.array_equal(H(seen[j]), seen_ref)
        r4 = TR.search_local_points(fr, mps, seen_ref, 3.0, 0.8, 0.5)
        g4 = dict(nmatches=int(nm2[j]), assigned=H(asg2[j, :n]), in_view=H(iv[j]), proj_x=H(px[j]), proj_y=H(py[j]), level=H(lv[j]),
                  view_cos=H(vc[j]), kp_point_out=H(kpo2[j, :n]), n_to_match=int(ntm[j]))
        d4 = TC.differences("local", r4, g4)
        assert not d4, "%s: the local-point search after the pose optimisation: %s" % (c.name, d4)


# ---------------------------------------------------------------- the C++ mirror (pilotguru_amd/host/orb_extractor.hpp)
CPP_DRIVER = r"""
// reads problems written by tests/test_pose_optimization.py and prints what pgorb::Optimizer::PoseOptimization returns: "inliers
// nmatchesMap status rounds", then the pose's floats as hex words, the flags, the slots and chi2 as hex words, or the exception
#include <cstdio>
#include <cstring>
#include <fstream>
#include "pilotguru_amd/host/orb_extractor.hpp"
using namespace pgorb;
template <class T> static void rd(std::ifstream& f, std::vector<T>& v) { int32_t n; f.read((char*)&n, 4); v.resize(n); if (n) f.read((char*)v.data(), (size_t)n * sizeof(T)); }
int main(int argc, char** argv)
{
    const bool run = argc > 1 && std::strcmp(argv[1], "run") == 0;        // "check": no context, the mirror's checks only
    ORBextractor* ext = run ? new ORBextractor(1000, 1.2f, 8, 20, 7, 640, 480) : nullptr;
    Optimizer opt(ext ? ext->context() : nullptr);
    for (int a = 2; a < argc; a++) {
        std::ifstream f(argv[a], std::ios::binary);
        Frame F; pgorb_kf_pose pose; std::vector<int32_t> slots; std::vector<pgorb_map_point> points; std::vector<uint8_t> obs; int32_t discard;
        rd(f, F.mvKeysUndistorted); f.read((char*)&pose, sizeof pose); rd(f, slots); rd(f, points); rd(f, obs); f.read((char*)&discard, 4);
        try {
            const PoseOptimizationResult r = opt.PoseOptimization(F, pose, slots, points, obs, discard != 0);
            std::printf("%d %d %d %d\n", r.inliers, r.nmatchesMap, r.info[0], r.info[1]);
            uint32_t w[sizeof(pgorb_kf_pose) / 4]; std::memcpy(w, &r.pose, sizeof w);
            for (size_t i = 0; i < sizeof w / 4; i++) std::printf(i ? " %08x" : "%08x", w[i]);
            std::printf("\n");
            for (size_t i = 0; i < r.outlier.size(); i++) std::printf(i ? " %d" : "%d", r.outlier[i]);
            std::printf("\n");
            for (size_t i = 0; i < r.kpPoint.size(); i++) std::printf(i ? " %d" : "%d", r.kpPoint[i]);
            std::printf("\n");
            for (size_t i = 0; i < r.chi2.size(); i++) { uint32_t u; std::memcpy(&u, &r.chi2[i], 4); std::printf(i ? " %08x" : "%08x", u); }
            std::printf("\n");
        } catch (const std::invalid_argument&) { std::printf("invalid_argument\n");
        } catch (const std::runtime_error&) { std::printf("runtime_error\n"); }
    }
    delete ext;
    return 0;
}
"""


def _cpp_driver(tmp_path):
    import subprocess
    root = os.path.dirname(HERE)
    src, exe = os.path.join(str(tmp_path), "pose_driver.cc"), os.path.join(str(tmp_path), "pose_driver")
    open(src, "w").write(CPP_DRIVER)
    lib = os.path.join(root, "pilotguru_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", root, src, "-o", exe, "-L", lib, "-lpgorb", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _write_problem(path, c, discard=False, **over):
    def arr(a, dt):
        a = np.ascontiguousarray(a, dt)
        return np.int32(a.shape[0]).tobytes() + a.tobytes()
    k = over.get("keys", PC.keypoints(c.keys_xy, c.octaves))
    pts = PC.table(over.get("points", c.points))
    with open(path, "wb") as f:
        f.write(arr(k, k.dtype) + np.asarray(over.get("pose", PC.pose_record(c.pose))).tobytes() + arr(over.get("kp_point", c.kp_point), np.int32) +
                arr(pts, pts.dtype) + arr(np.zeros(0, np.uint8) if c.has_obs is None else c.has_obs, np.uint8) + np.int32(discard).tobytes())


def _run_driver(exe, mode, paths):
    import subprocess
    return subprocess.run([exe, mode] + paths, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines()


def test_cpp_mirror_rejects_bad_inputs_before_calling_the_library(tmp_path):
    """pgorb::Optimizer::PoseOptimization throws std::invalid_argument for every input pgorb_pose_optimization would refuse, before
    any pointer reaches the library; well-formed input reaches it (a NULL context here, so PGORB_E_ARG comes back as
    std::runtime_error)."""
    exe = _cpp_driver(tmp_path)
    c = cases()["ten"]
    bad = _bad_inputs(c) + [("kp_point too short", dict(kp_point=c.kp_point[:-1]))]
    paths = [os.path.join(str(tmp_path), "p%d.bin" % i) for i in range(len(bad) + 1)]
    _write_problem(paths[0], c)
    for path, (_, over) in zip(paths[1:], bad):
        _write_problem(path, c, **over)
    out = _run_driver(exe, "check", paths)
    assert out[0] == "runtime_error"
    assert out[1:] == ["invalid_argument"] * len(bad), [w for (w, _), o in zip(bad, out[1:]) if o != "invalid_argument"]


@pytest.mark.gpu
def test_gpu_cpp_mirror_equals_the_single_call(ext, tmp_path):
    exe = _cpp_driver(tmp_path)
    names = ["no_obs_points", "few_2", "z_zero"]
    c = cases()["ten"]
    octs = c.octaves.copy()
    octs[np.flatnonzero(c.kp_point >= 0)[0]] = PC.NLEVELS
    paths = [os.path.join(str(tmp_path), "%s.bin" % n) for n in names + ["octave"]]
    for n, path in zip(names, paths):
        _write_problem(path, cases()[n], discard=True)
    _write_problem(paths[-1], c, keys=PC.keypoints(c.keys_xy, octs))
    out = _run_driver(exe, "run", paths)
    assert out[-1] == "invalid_argument"
    for i, n in enumerate(names):
        g = PC.run_gpu(cases()[n], ext, discard=True)
        head, pose, fl, kp, chi = out[5 * i:5 * i + 5]
        assert [int(x) for x in head.split()] == [g["ret"], g["nmatches_map"], g["status"], g["rounds"]], n
        assert bytes.fromhex("".join(w[6:8] + w[4:6] + w[2:4] + w[0:2] for w in pose.split())) == g["pose_bytes"], n
        assert [int(x) for x in fl.split()] == list(g["outlier"]) and [int(x) for x in kp.split()] == list(g["kp_point_out"]), n
        assert [int(x, 16) for x in chi.split()] == list(g["chi2"].view(np.uint32)), n
