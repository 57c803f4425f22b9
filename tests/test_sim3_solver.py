"""pgorb_sim3_solver (pilotguru_amd/csrc/sim3.hip): Sim3Solver on the device, against the plain reference of
tests/sim3_reference.py on the loop candidates of tests/sim3_cases.py.

The reference is UNPINNED to OpenCV (2.4.9 cannot be built where the suite runs); the CPU tests below anchor it: Horn on three
points against the Umeyama / SVD solution of numpy, noise-free scenes that return the generating Sim3 from any non-degenerate
triple, the closed form of the swap-with-back selection against the literal list, and the iteration cap -- the library's host
table against a direct evaluation for every N in range.

Tolerances.  Integers and flags are compared exactly.  The float outputs get, per case and output, the larger of 2 float ulps at
the output's scale and 16 x the spread the reference shows between its arithmetic forms (tests/golden/sim3_spread.json, written
by tests/golden/make_sim3_spread.py): sim3_cases.bounds.  Every case meets the case condition (sim3_cases.condition) with the
window that follows from the same file, so no inlier flag can hang on the last bits of an error.

One mutant of the issue's list, "N == minInliers not forced to one iteration", cannot change any output: without the special
case the reference's own expression gives log(1 - 1) = -inf, a quotient of +0, ceil 0 and max(1, 0) = 1 -- one iteration all the
same.  test_n_equals_min_inliers_special_case_is_redundant shows that for every N instead."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim3_cases as SC  # noqa: E402
import sim3_reference as SR  # noqa: E402

f32, f64 = np.float32, np.float64
CASE_NAMES = ["few_19", "n20_cap_one", "n21_clean", "n64_outliers", "n65_outliers", "n257_outliers", "heavy_outliers", "scale_free",
              "scale_fixed", "scale_fixed_unit", "two_cameras", "mixed_octaves", "sparse_slots", "degenerate_triples", "late_success",
              "resume_carried_best"]
NEW_SYMBOLS = ["pgorb_sim3_solver", "pgorb_sim3_solver_batch_device", "pgorb_sim3_max_iterations"]
BATCH_CAP = 263                      # one cap_per_frame for every case: above the largest key frame (257), no multiple of 64
EQUIVALENT_MUTANTS = ("n_equals_min_not_special",)
_cache = {}


def cases():
    return {c.name: c for c in SC.all_cases()}


def want(name):
    return SC.reference(cases()[name])


def recorded():
    if "spread" not in _cache:
        _cache["spread"] = SC.recorded_spread()
    return _cache["spread"]


# ---------------------------------------------------------------- CPU
def test_symbols_and_mirror_exist():
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(HERE), "include", "pgorb.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in _lib.SYMBOLS and (s + "(") in header
    for m in ("SetRansacParameters", "iterate", "find", "GetEstimatedRotation", "GetEstimatedTranslation", "GetEstimatedScale",
              "iterate_batch_device"):
        assert callable(getattr(pg.Sim3Solver, m))
    assert (pg.S3_FEW, pg.S3_FOUND, pg.S3_NO_MORE, pg.S3_INFO, pg.SIM3_MAX_ITERATIONS) == (SR.S3_FEW, SR.S3_FOUND, SR.S3_NO_MORE, 8, 1024)
    assert pg.SIM3_PARAMS_DTYPE.itemsize == 28 and pg.SIM3_ESTIMATE_DTYPE.itemsize == 52
    hpp = open(os.path.join(os.path.dirname(HERE), "pilotguru_amd", "host", "orb_extractor.hpp")).read()
    assert "class Sim3Solver" in hpp


def test_case_list_is_what_the_tests_name():
    assert [c.name for c in SC.all_cases()] == CASE_NAMES
    N = {n: want(n)["N"] for n in CASE_NAMES}
    assert [N[n] for n in CASE_NAMES[:6]] == [19, 20, 21, 64, 65, 257]
    c = cases()["sparse_slots"]
    assert c.n1 > N["sparse_slots"] and c.bad.any() and (c.matches12 < 0).any() and (c.kf_point1 < 0).any() and (c.kf_point2 < 0).any()
    assert max(max(c.n1, c.n2) for c in SC.all_cases()) < BATCH_CAP and BATCH_CAP % 64 != 0
    assert len(set(int(o) for o in cases()["mixed_octaves"].octaves1)) == SC.NLEVELS
    assert int(cases()["n21_clean"].draws[0, 0]) == 2 ** 31 - 1
    assert len(SC.batch_groups(SC.all_cases())) == 2, "fix_scale 0 and fix_scale 1: two batched calls cover every case"


def test_cases_reach_what_they_are_built_for():
    w = want
    assert w("few_19")["status"] == SR.S3_FEW and w("few_19")["its_after"] == 0 and w("few_19")["best_iteration"] == -1
    a = w("n20_cap_one")
    assert (a["cap"], a["status"], a["best_inliers"], a["ret"], a["its_after"]) == (1, SR.S3_NO_MORE, 20, 0, 1)
    assert w("n21_clean")["status"] == SR.S3_FOUND and w("n21_clean")["best_iteration"] == 0 and w("n21_clean")["ret"] == 21
    for n in ("n64_outliers", "n65_outliers", "n257_outliers"):
        assert w(n)["status"] == SR.S3_FOUND and w(n)["best_iteration"] == 3 and w(n)["ret"] == int(cases()[n].good.sum())
    # no success inside the cap; the maximum is reached more than once and `best` is the last of them
    tr = []
    h = SC.run_reference(cases()["heavy_outliers"], trace=tr)
    counts = [x[5] for x in tr]
    assert h["status"] == SR.S3_NO_MORE and len(counts) == h["cap"] == h["its_after"] and max(counts) <= 20
    top = [t for t, k in enumerate(counts) if k == max(counts)]
    assert len(top) >= 2 and h["best_iteration"] == top[-1] and h["best_inliers"] == max(counts)
    # scale 1.7: found with the scale free, hopeless with the scale fixed; scale 1: found with the scale fixed
    assert w("scale_free")["status"] == w("scale_fixed_unit")["status"] == SR.S3_FOUND and w("scale_fixed")["status"] == SR.S3_NO_MORE
    assert abs(float(w("scale_free")["found_s"]) - 1.7) < 1e-3 and float(w("scale_fixed_unit")["found_s"]) == 1.0
    assert w("two_cameras")["status"] == SR.S3_FOUND and cases()["two_cameras"].pose2["fx"] != cases()["two_cameras"].pose1["fx"]
    # the resumed solver: iteration 1 has more than min_inliers and fewer than the carried best, so iteration 2 returns
    c = cases()["resume_carried_best"]
    tr = []
    r = SC.run_reference(c, trace=tr)
    assert [x[0] for x in tr] == [1, 2] and c.params["min_inliers"] < tr[0][5] < c.params["best_inliers_in"] <= tr[1][5]
    assert r["status"] == SR.S3_FOUND and r["best_iteration"] == 2 and r["its_after"] == 3
    # the degenerate triples: identical clouds give no finite hypothesis, the z = 0 correspondence is never an inlier
    c = cases()["degenerate_triples"]
    tr = []
    r = SC.run_reference(c, trace=tr)
    t0 = tr[0]
    assert np.isnan(t0[2].R).all() and t0[5] == 0 and not np.isfinite(t0[3]).any()
    P = np.array([SR.correspondences(c.octaves1, c.pose1, c.kf_point1, c.octaves2, c.pose2, c.kf_point2, c.matches12, c.points, c.bad,
                                     SC.SIGMA2).X1[k] for k in tr[1][1]], f64)
    assert np.linalg.svd(P - P.mean(0), compute_uv=False)[1] < 1e-5, "iteration 1 draws three collinear points"
    C0 = SR.correspondences(c.octaves1, c.pose1, c.kf_point1, c.octaves2, c.pose2, c.kf_point2, c.matches12, c.points, c.bad, SC.SIGMA2)
    z0 = np.flatnonzero(C0.X1[:, 2] == 0)
    assert len(z0) == 1 and int(z0[0]) in tr[2][1] and not np.isfinite(C0.p1[z0[0]]).all()
    assert r["status"] == SR.S3_FOUND and r["best_iteration"] == 3 and r["inlier"][C0.i1[z0[0]]] == 0
    assert w("late_success")["best_iteration"] == 7


@pytest.mark.parametrize("mutant", sorted(SR.MUTANTS))
def test_every_mutant_changes_a_compared_output(mutant):
    """On at least one case -- but for the one mutant that is the reference itself in other words (the module docstring): for it
    the test holds that the iteration cap, the only thing the switch touches, is the same for every N."""
    rules = SR.MUTANTS[mutant]
    if mutant in EQUIVALENT_MUTANTS:
        assert all(SR.max_iterations(0.99, 20, 300, N, rules) == SR.max_iterations(0.99, 20, 300, N) for N in range(0, 400))
        return
    for n in CASE_NAMES:
        if SC.differences(cases()[n], want(n), SC.run_reference(cases()[n], rules=rules), recorded()[n])[0]:
            return
    pytest.fail("no case notices the mutant %s" % mutant)


def test_n_equals_min_inliers_special_case_is_redundant():
    rules = SR.MUTANTS["n_equals_min_not_special"]
    for m in (3, 6, 20, 100):
        assert SR.max_iterations(0.99, m, 300, m, rules) == SR.max_iterations(0.99, m, 300, m) == 1


def test_iteration_cap_table_equals_a_direct_evaluation():
    """The library's host expression (what its context table holds) against Python's libm for every N in range.  nIterations is an
    int: a quotient of 2^31 or more converts to INT_MIN on x86-64 (cvttsd2si), and max(1, min(INT_MIN, maxIterations)) is 1 -- with
    20 inliers asked of more than about 15500 correspondences the reference runs ONE iteration, and so does the library."""
    from pilotguru_amd import _lib
    L = _lib.lib()
    for prob, m, mx in ((0.99, 20, 300), (0.99, 6, 300), (0.5, 3, 1024), (0.999, 20, 40)):
        for N in range(0, SC.MAX_N + 1):
            if N < m or N == m:
                direct = 1
            else:
                eps = float(f32(m) / f32(N))
                v = math.ceil(math.log(1.0 - float(f32(prob))) / math.log(1.0 - math.pow(eps, 3)))
                direct = max(1, min(int(v) if v < 2.0 ** 31 else -2 ** 31, mx))
            got = L.pgorb_sim3_max_iterations(prob, m, mx, N)
            assert got == direct == SR.max_iterations(prob, m, mx, N), (prob, m, mx, N, got, direct)
    assert [SR.max_iterations(0.99, 20, 300, N) for N in (21, 30, 64, 65, 257, 15000, 16000)] == [3, 14, 149, 156, 300, 300, 1]


def test_closed_form_triple_equals_the_list():
    rng = np.random.RandomState(5)
    for N in (3, 4, 5, 20, 21, 64, 257, 16000):
        for d in rng.randint(0, 2 ** 31, (400, 3)):
            assert SR.triple_closed(d, N) == SR.triple_list(d, N)
        for d in ((0, 0, 0), (2 ** 31 - 1,) * 3, (2 ** 31 - 1, 0, 2 ** 31 - 1), (0, 2 ** 31 - 1, 0)):
            assert SR.triple_closed(d, N) == SR.triple_list(d, N) and len(set(SR.triple_list(d, N))) == 3
    assert SR.random_int(2 ** 31 - 1, 257) == 256 and SR.random_int(0, 257) == 0


def _umeyama(X1, X2):
    """s, R, t minimising |X1 - (s R X2 + t)|^2 over the rows (Umeyama 1991), in double."""
    c1, c2 = X1.mean(0), X2.mean(0)
    A, B = X1 - c1, X2 - c2
    U, S, Vt = np.linalg.svd(A.T @ B / len(X1))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / (B ** 2).sum() * len(X1)
    return s, R, c1 - s * R @ c2


def test_anchor_horn_equals_umeyama_on_three_points():
    rng = np.random.RandomState(17)
    for k in range(40):
        R0, t0, s0 = SC.rotation(rng.uniform(-1.5, 1.5, 3)), rng.uniform(-2, 2, 3), rng.uniform(0.5, 2.0)
        X2 = rng.uniform(-2, 2, (3, 3)) + np.array([0, 0, 5.0])
        X1 = (s0 * X2 @ R0.T + t0).astype(f32)
        X2 = X2.astype(f32)
        if np.linalg.svd(X2 - X2.mean(0), compute_uv=False)[1] < 0.3:
            continue
        s, R, t = _umeyama(X1.astype(f64), X2.astype(f64))
        for forms in SR.FORMS.values():
            T = SR.horn(X1.T, X2.T, False, forms)
            assert np.abs(T.R - R).max() < 2e-5 and abs(float(T.s) - s) < 2e-5 * s and np.abs(T.t - t).max() < 2e-4, k
            assert np.abs(T.sR12 - s * R).max() < 5e-5 and np.abs(T.sR21 - R.T / s).max() < 5e-5 and np.abs(T.t21 + (R.T / s) @ t).max() < 3e-4
        Tf = SR.horn(X1.T, X2.T, True)
        assert float(Tf.s) == 1.0 and np.abs(Tf.R - R).max() < 2e-5


def test_anchor_noise_free_scenes_return_the_generating_sim3():
    rng = np.random.RandomState(3)
    for name in ("n21_clean", "scale_free", "two_cameras"):
        c = cases()[name]
        Rs, ts, s = c.true
        C0 = SR.correspondences(c.octaves1, c.pose1, c.kf_point1, c.octaves2, c.pose2, c.kf_point2, c.matches12, c.points, c.bad, SC.SIGMA2)
        good = np.flatnonzero(c.good)
        tried = 0
        while tried < 25:
            tri = rng.choice(good, 3, replace=False)
            P = C0.X2[tri].astype(f64)
            if np.linalg.svd(P - P.mean(0), compute_uv=False)[1] < 0.3:
                continue                                                # nearly collinear: the rotation about the line is not determined
            tried += 1
            T = SR.horn(C0.X1[tri].T, C0.X2[tri].T)
            assert np.abs(T.R - Rs).max() < 1e-4 and abs(float(T.s) - s) < 1e-4 * s and np.abs(T.t - ts).max() < 1e-3, (name, tri)
            e1, e2 = SR.errors(T, C0)
            assert (e1[good] < 0.05).all() and (e2[good] < 0.05).all()


def test_spread_file_is_up_to_date():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_sim3_spread
    now = make_sim3_spread.measure()
    assert sorted(now) == sorted(recorded()) == sorted(CASE_NAMES)
    # one of the forms goes through LAPACK (numpy.linalg.eigh), whose last bits may differ between builds: within a factor of two
    # (the bounds take 16 x), above a floor of an eighth of a float ulp
    floor = SC.ULP1 / 8.0
    for n in CASE_NAMES:
        for k in SC.FLOAT_OUTPUTS:
            a, b = now[n][k], recorded()[n][k]
            assert a <= 2.0 * b + floor and b <= 2.0 * a + floor, "run tests/golden/make_sim3_spread.py (%s, %s: %g, recorded %g)" % (n, k, a, b)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_case_meets_the_case_condition(name):
    bad = SC.condition(cases()[name], recorded()[name])
    assert not bad, "%s: rebuild the case with other seeds or draws: %s" % (name, bad)


def test_chain_scenes_meet_the_case_condition():
    for seed in SC.CHAIN_SEEDS:
        c, b, draws, m12, sc, r, (n3, s12) = _chain(seed)
        assert not SC.condition(sc, SC.spread(sc)), seed
        assert 100 <= len(c.slots1) <= 140 and r["status"] == SR.S3_FOUND and 20 < r["ret"] < r["N"] and n3 > 0


def _chain(seed):
    if ("chain", seed) not in _cache:
        _cache[("chain", seed)] = SC.chain_reference(seed)
    return _cache[("chain", seed)]


def _windows(c, step):
    """Chained calls of niterations = 5 from mnIterations = 0 to the end, each through step(case) -> result; returns the last
    result, the last non-empty best and the number of calls."""
    its, best_in, best, calls = 0, 0, None, 0
    while True:
        r = step(c.variant(params=dict(first_iteration=its, best_inliers_in=best_in, niterations=5)))
        calls += 1
        assert r["its_after"] > its or r["status"] & (SR.S3_FEW | SR.S3_NO_MORE)
        its, best_in = r["its_after"], r["best_inliers"]
        if r["best_iteration"] >= 0:
            best = (r["best_R"].tobytes(), r["best_t"].tobytes(), f32(r["best_s"]).tobytes(), r["best_iteration"])
        if r["status"] & (SR.S3_FEW | SR.S3_FOUND | SR.S3_NO_MORE):
            return r, best, calls


WINDOW_FIELDS = ("ret", "status", "its_after", "ninliers", "best_inliers", "inlier", "matches12_out", "already1", "already2", "found_R",
                 "found_t", "found_s", "sR12", "t12", "sR21", "t21")


def _same_as_find(c, step, full):
    r, best, calls = _windows(c, step)
    for k in WINDOW_FIELDS:
        assert np.asarray(r[k]).tobytes() == np.asarray(full[k]).tobytes(), (c.name, k)
    if full["best_iteration"] < 0:
        assert best is None, c.name
    else:
        assert best == (full["best_R"].tobytes(), full["best_t"].tobytes(), f32(full["best_s"]).tobytes(), full["best_iteration"]), c.name
    return calls


def test_windows_of_five_chained_equal_one_find_in_the_reference():
    assert _same_as_find(cases()["heavy_outliers"], SC.run_reference, want("heavy_outliers")) == 7
    assert _same_as_find(cases()["late_success"], SC.run_reference, want("late_success")) == 2
    assert _same_as_find(cases()["few_19"], SC.run_reference, want("few_19")) == 1


# ---------------------------------------------------------------- malformed input
class _KF:
    def __init__(self, ext, octaves):
        self.ext, self.N, self.mvKeysUndistorted = ext, len(octaves), SC.keypoints(octaves)[:len(octaves)]


def _table(c):
    import pilotguru_amd as pg
    n = len(c.points)
    return pg.MapPointTable(SC.table(c.points)[:n], np.zeros((n, 32), np.uint8), c.bad, np.arange(n + 1, dtype=np.int32), np.zeros(max(n, 1), np.uint64))


def _mirror(c, ext=None):
    """The Python mirror on a case: the solver after one iterate(niterations) from the case's mnIterations / mnBestInliers."""
    import pilotguru_amd as pg
    s = pg.Sim3Solver(_KF(ext, c.octaves1), _KF(ext, c.octaves2), SC.pose_record(c.pose1), SC.pose_record(c.pose2), c.kf_point1, c.kf_point2,
                      c.matches12, _table(c), bool(c.params["fix_scale"]), draws=c.draws)
    s.SetRansacParameters(c.params["probability"], c.params["min_inliers"], c.params["max_iterations"])
    s.mnIterations, s.mnBestInliers = c.params["first_iteration"], c.params["best_inliers_in"]
    return s, s.iterate(c.params["niterations"])


def _bad_arrays(c):
    """(what, the case with it) for every array input the checked call must refuse: see include/pgorb.h."""
    used = np.flatnonzero((c.matches12 >= 0) & (c.kf_point1 >= 0))
    used = used[c.kf_point2[c.matches12[used]] >= 0]
    out = []

    def put(what, field, idx, value, dt=np.int32):
        a = np.array(getattr(c, field), dt, copy=True)
        a[idx] = value
        out.append((what, c.variant(**{field: a})))
    put("kf_point1 == npoints", "kf_point1", 0, len(c.points))
    put("kf_point1 < -1", "kf_point1", 1, -2)
    put("kf_point2 == npoints", "kf_point2", 2, len(c.points))
    put("matches12 == n2", "matches12", 3, c.n2)
    put("matches12 < -1", "matches12", 4, -2)
    put("a draw of 2^31", "draws", (c.params["max_iterations"] - 1, 2), 2 ** 31, np.uint32)
    for k, v in (("Tcw", np.nan), ("Tcw", np.inf), ("fx", np.nan), ("cy", np.inf)):
        for which in ("pose1", "pose2"):
            P = dict(getattr(c, which))
            if k == "Tcw":
                P["Tcw"] = P["Tcw"].copy()
                P["Tcw"][7] = v
            else:
                P[k] = f32(v)
            out.append(("%s %s = %r" % (which, k, v), c.variant(**{which: P})))
    pts = c.points.copy()
    pts[c.kf_point2[c.matches12[used[2]]], 1] = np.nan
    out.append(("a referenced point is NaN", c.variant(points=pts)))
    return out, used


BAD_PARAMS = [dict(min_inliers=2), dict(probability=0.0), dict(probability=1.0), dict(probability=float("nan")), dict(max_iterations=0),
              dict(first_iteration=-1), dict(niterations=0)]


def test_mirror_refuses_malformed_input_without_a_device():
    """Pure host checks: every malformed input is a ValueError before any library call; well-formed input gets past them (to the
    missing device).  An unreferenced point may be anything.  The library makes the same checks itself (PGORB_E_ARG):
    test_gpu_library_and_mirrors_refuse_malformed_input."""
    import pilotguru_amd as pg
    c = cases()["sparse_slots"]
    with pytest.raises(AttributeError):
        _mirror(c)
    bad, used = _bad_arrays(c)
    pts = np.concatenate([c.points, np.full((1, 3), np.nan, f32)])      # a point no slot names
    with pytest.raises(AttributeError):
        _mirror(c.variant(points=pts, bad=np.append(c.bad, 0).astype(np.uint8)))
    for what, v in bad:
        with pytest.raises(ValueError):
            _mirror(v)
            pytest.fail(what)
    with pytest.raises(ValueError):
        _mirror(c.variant(matches12=c.matches12[:-1]))
    for prm in BAD_PARAMS + [dict(max_iterations=1025)]:
        p = dict(c.params, **prm)
        with pytest.raises(ValueError):
            pg.Sim3Solver.check_params("t", p["probability"], p["min_inliers"], p["max_iterations"], p["first_iteration"], p["niterations"])
            pytest.fail(repr(prm))
    pg.Sim3Solver.check_params("t", 0.99, 20, 300, 0, 5, c.draws)
    with pytest.raises(ValueError):
        pg.Sim3Solver.check_params("t", 0.99, 20, 300, 0, 5, c.draws[:299])


def test_batched_wrapper_refuses_mistyped_or_short_tensors_without_a_device():
    """The wrapper takes the pair count and the row lengths from element counts: an index tensor that is not int32 (a byte view, say)
    would make it launch more pairs than there are.  Checked before anything reaches the library."""
    import torch
    import pilotguru_amd as pg
    from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE
    B, cap, nf = 2, 8, 4
    I = lambda *sh: torch.zeros(sh, dtype=torch.int32)  # noqa: E731
    U = lambda *sh: torch.zeros(sh, dtype=torch.uint8)  # noqa: E731
    good = dict(d_kps=U(nf, cap, KEYPOINT_DTYPE.itemsize), d_n=I(nf), d_pair_kf1=I(B), d_pair_kf2=I(B), d_pose=U(nf, KF_POSE_DTYPE.itemsize),
                d_kf_point=I(nf, cap), d_matches12=I(B, cap), d_points=U(5, 32), d_point_bad=U(5), d_draws=I(B, 300, 3))

    def call(**over):
        a = dict(good, **over)
        return pg.Sim3Solver.iterate_batch_device(None, a["d_kps"], a["d_n"], cap, a["d_pair_kf1"], a["d_pair_kf2"], a["d_pose"], a["d_kf_point"],
                                                  a["d_matches12"], 5, a["d_points"], a["d_point_bad"], a["d_draws"])
    with pytest.raises((AttributeError, RuntimeError)) as e:            # well-formed: past the checks, to the missing device or extractor
        call()
    assert not isinstance(e.value, ValueError)
    for over in (dict(d_pair_kf1=U(B * 4)), dict(d_pair_kf2=I(B + 1)), dict(d_matches12=U(B, cap * 4)), dict(d_matches12=I(B, cap + 1)),
                 dict(d_draws=I(B, 299, 3)), dict(d_draws=U(B, 300, 3)), dict(d_kf_point=I(nf, cap - 1)), dict(d_kps=U(nf, cap, 27)),
                 dict(d_pose=U(nf - 1, KF_POSE_DTYPE.itemsize)), dict(d_points=U(4, 32)), dict(d_point_bad=U(4)), dict(d_n=U(nf * 4))):
        with pytest.raises(ValueError):
            call(**over)
            pytest.fail(repr({k: tuple(v.shape) for k, v in over.items()}))


def test_null_context_is_an_argument_error():
    from pilotguru_amd import _lib
    L = _lib.lib()
    z = np.zeros(64, np.float32)
    p = C.c_void_p(z.ctypes.data)
    assert L.pgorb_sim3_solver(None, p, 0, p, p, p, 0, p, p, p, 0, p, None, p, p, p, p, p, p, p, None, None, None) == _lib.PGORB_E_ARG
    assert L.pgorb_sim3_solver_batch_device(None, p, p, 1, p, p, 0, p, p, p, 0, p, None, p, None, None, p, p, p, p, p, p, None, None, None, None,
                                            None) == _lib.PGORB_E_ARG


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(1000, 1.2, SC.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=4)
    assert np.array_equal(np.asarray(e.GetScaleSigmaSquares(), f32)[:SC.NLEVELS], SC.SIGMA2)
    yield e
    e.close()


def _check(c, w, got, what, spread):
    assert not isinstance(got, int), "%s (%s): error %r" % (c.name, what, got)
    bad, d = SC.differences(c, w, got, spread)
    print("%s (%s): status %d, iterations %d, inliers %d of %d, scaled differences %s against %s" % (
        c.name, what, got["status"], got["its_after"], got["ninliers"], got["N"], d, SC.bounds(spread)))
    assert not bad, "%s (%s): %s differ from the reference" % (c.name, what, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_single_call_equals_the_reference(ext, name):
    _check(cases()[name], want(name), SC.run_gpu(cases()[name], ext), "single call", recorded()[name])


@pytest.mark.gpu
def test_gpu_batch_equals_the_reference_and_its_singles_byte_for_byte(ext):
    """Every case in a batch padded to one cap_per_frame (one call per value of fix_scale: the parameter block is one for all
    pairs) -- and the determinism contract: the same bytes on a repeat, on a second stream and with the pairs in another order."""
    import torch
    seen = 0
    for grp in SC.batch_groups(SC.all_cases()):
        res = SC.run_gpu_batch(grp, ext, BATCH_CAP)
        for c, r in zip(grp, res):
            _check(c, want(c.name), r, "batched", recorded()[c.name])
            assert r["tail_ok"], "%s: the entries past n are not those of no correspondence" % c.name
            assert SC.run_gpu(c, ext)["raw"] == r["raw"], "%s: the single call and the batch differ" % c.name
        raw = [r["raw"] for r in res]
        assert [r["raw"] for r in SC.run_gpu_batch(grp, ext, BATCH_CAP)] == raw, "a repeated call gives other bytes"
        assert [r["raw"] for r in SC.run_gpu_batch(grp, ext, BATCH_CAP, stream=torch.cuda.Stream())] == raw, "a second stream gives other bytes"
        perm = list(np.random.RandomState(len(grp)).permutation(len(grp)))
        got = SC.run_gpu_batch(grp, ext, BATCH_CAP, order=perm)
        assert [got[perm.index(j)]["raw"] for j in range(len(grp))] == raw, "a pair's result depends on its place in the batch"
        seen += len(grp)
    assert seen == len(CASE_NAMES)


@pytest.mark.gpu
def test_gpu_windows_of_five_chained_equal_one_find(ext):
    step = lambda c: SC.run_gpu(c, ext)  # noqa: E731
    for name, calls in (("heavy_outliers", 7), ("late_success", 2), ("few_19", 1)):
        full = SC.run_gpu(cases()[name], ext)
        _check(cases()[name], want(name), full, "find", recorded()[name])
        assert _same_as_find(cases()[name], step, full) == calls


@pytest.mark.gpu
def test_gpu_python_mirror_equals_the_single_call(ext):
    """... through its reference surface: find(), and iterate(5) called again on the same solver."""
    for name in ("n65_outliers", "resume_carried_best", "heavy_outliers", "few_19"):
        c, g = cases()[name], SC.run_gpu(cases()[name], ext)
        s, (T12, no_more, inl, n) = _mirror(c, ext)
        assert n == g["ret"] and np.array_equal(inl.astype(np.uint8), g["inlier"]) and (T12 is not None) == bool(g["status"] & SR.S3_FOUND)
        assert no_more == bool(g["status"] & (SR.S3_FEW | SR.S3_NO_MORE)) and s.mnIterations == g["its_after"] and s.mnBestInliers == g["best_inliers"]
        assert np.array_equal(s.matches12_out, g["matches12_out"]) and np.array_equal(s.already1, g["already1"]) and np.array_equal(s.already2, g["already2"])
        if T12 is not None:
            assert T12[:3, :3].tobytes() == g["sR12"].tobytes() and T12[:3, 3].tobytes() == g["t12"].tobytes() and T12[3].tolist() == [0, 0, 0, 1]
        if g["best_iteration"] >= 0:
            assert s.GetEstimatedRotation().tobytes() == g["best_R"].tobytes() and s.GetEstimatedTranslation().tobytes() == g["best_t"].tobytes()
            assert f32(s.GetEstimatedScale()) == g["best_s"]
    # LoopClosing's use: iterate(5) until bNoMore or a result
    c = cases()["late_success"].variant(params=dict(niterations=5))
    s, (T12, no_more, inl, n) = _mirror(c, ext)
    assert T12 is None and not no_more and s.mnIterations == 5
    T12, no_more, inl, n = s.iterate(5)
    g = SC.run_gpu(cases()["late_success"], ext)
    assert T12 is not None and n == g["ret"] and s.mnIterations == g["its_after"] == 8 and np.array_equal(inl.astype(np.uint8), g["inlier"])


@pytest.mark.gpu
def test_gpu_library_and_mirrors_refuse_malformed_input(ext):
    from pilotguru_amd import _lib
    c = cases()["sparse_slots"]
    assert SC.run_gpu(c, ext)["ret"] == want("sparse_slots")["ret"]
    bad, used = _bad_arrays(c)
    o1 = c.octaves1.copy()
    o1[used[0]] = SC.NLEVELS
    o2 = c.octaves2.copy()
    o2[c.matches12[used[1]]] = -1
    bad += [("a used KF1 octave outside the levels", c.variant(octaves1=o1)), ("a used KF2 octave outside the levels", c.variant(octaves2=o2))]
    for what, v in bad:
        assert SC.run_gpu(v, ext) == _lib.PGORB_E_ARG, what
        with pytest.raises(ValueError):
            _mirror(v, ext)
            pytest.fail(what)
    for prm in BAD_PARAMS:
        assert SC.run_gpu(c, ext, **prm) == _lib.PGORB_E_ARG, prm
        with pytest.raises(ValueError):
            _mirror(c.variant(params=prm), ext)
            pytest.fail(repr(prm))
    # negative counts and NULL arrays that are read
    L, h = ext._L, ext._h
    z = np.zeros(4096, np.int32)
    p = C.c_void_p(z.ctypes.data)
    prm = SC.params_record(c.params)
    q = C.c_void_p(prm.ctypes.data)
    for n1, n2, npnt in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert L.pgorb_sim3_solver(h, p, n1, p, p, p, n2, p, p, p, npnt, p, None, q, p, p, p, p, p, p, None, None, None) == _lib.PGORB_E_ARG
    assert L.pgorb_sim3_solver(h, p, 0, p, p, p, 0, p, p, p, 0, p, None, None, p, p, p, p, p, p, None, None, None) == _lib.PGORB_E_ARG
    assert L.pgorb_sim3_solver(h, p, 0, p, p, p, 0, p, p, p, 0, p, None, q, None, p, p, p, p, p, None, None, None) == _lib.PGORB_E_ARG
    assert L.pgorb_sim3_solver(h, None, 4, p, p, p, 4, p, p, p, 0, p, None, q, p, p, p, p, p, p, None, None, None) == _lib.PGORB_E_ARG
    # an octave outside the levels and a non-finite point where there is no correspondence are not read
    free = c.octaves1.copy()
    free[np.flatnonzero(c.matches12 < 0)[0]] = 99
    assert SC.run_gpu(c.variant(octaves1=free), ext)["raw"] == SC.run_gpu(c, ext)["raw"]


@pytest.mark.gpu
def test_gpu_limits(ext):
    """16000 keypoints a key frame run; 16001 and max_iterations = 1025 are PGORB_E_LIMIT, in both forms."""
    from pilotguru_amd import _lib
    import torch
    c = cases()["n21_clean"]
    n = SC.MAX_N
    pad = lambda a, m, fill: np.concatenate([np.asarray(a), np.full(m - len(a), fill, np.asarray(a).dtype)])  # noqa: E731
    big = c.variant(octaves1=pad(c.octaves1, n, 0), kf_point1=pad(c.kf_point1, n, -1), matches12=pad(c.matches12, n, -1),
                    octaves2=pad(c.octaves2, n, 0), kf_point2=pad(c.kf_point2, n, -1))
    g = SC.run_gpu(big, ext)
    w = want("n21_clean")
    assert g["ret"] == w["ret"] and np.array_equal(g["inlier"][:c.n1], w["inlier"]) and not g["inlier"][c.n1:].any()
    assert g["found_R"].tobytes() == SC.run_gpu(c, ext)["found_R"].tobytes()
    over = c.variant(octaves1=pad(c.octaves1, n + 1, 0), kf_point1=pad(c.kf_point1, n + 1, -1), matches12=pad(c.matches12, n + 1, -1))
    assert SC.run_gpu(over, ext) == _lib.PGORB_E_LIMIT
    d = np.zeros((1025, 3), np.uint32)
    assert SC.run_gpu(c.variant(draws=d), ext, max_iterations=1025) == _lib.PGORB_E_LIMIT
    assert not isinstance(SC.run_gpu(c.variant(draws=d), ext, max_iterations=1024), int)
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = C.c_void_p(t.data_ptr())
    for cap, mx in ((n + 1, 300), (64, 1025)):
        prm = SC.params_record(dict(c.params, max_iterations=mx))
        assert ext._L.pgorb_sim3_solver_batch_device(ext._h, p, p, cap, p, p, 1, p, p, p, 1, p, None, C.c_void_p(prm.ctypes.data), None, None, p, p, p,
                                                     p, p, p, None, None, None, None, None) == _lib.PGORB_E_LIMIT


# ---------------------------------------------------------------- the chain of ComputeSim3 on a resident batch
@pytest.mark.gpu
def test_gpu_chain_bow_solver_sim3_search_on_a_resident_batch(ext):
    """pgorb_search_by_bow_keyframes_batch_device -> pgorb_sim3_solver_batch_device -> pgorb_search_by_sim3_batch_device on three
    key-frame pairs of about 120 keypoints: d_matches12 goes from the first call to the second, d_found_sim3, d_already1 and
    d_already2 from the second to the third, with no download in between; every stage against its reference."""
    import torch
    import loop_cases as LC
    import pilotguru_amd as pg
    from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, SIM3_DTYPE, SIM3_ESTIMATE_DTYPE
    ch = [_chain(seed) for seed in SC.CHAIN_SEEDS]
    L, h = ext._L, ext._h
    B = len(ch)
    nf = 2 * B
    cap = max(max(len(c.slots1), len(c.slots2)) for c, *_ in ch) + 5
    kp = np.zeros((nf, cap), KEYPOINT_DTYPE)
    ds = np.full((nf, cap, 32), 0xFF, np.uint8)
    n, nfv = np.zeros(nf, np.int32), np.zeros(nf, np.int32)
    fn, ff, fs = np.zeros((nf, cap), np.uint32), np.zeros((nf, cap), np.uint32), np.zeros((nf, cap + 1), np.int32)
    v1, v2 = np.zeros((B, cap), np.uint8), np.zeros((B, cap), np.uint8)
    slots = np.full((nf, cap), -1, np.int32)
    poses = np.zeros(nf, KF_POSE_DTYPE)
    draws = np.zeros((B, 300, 3), np.uint32)
    allpts, off = [], []
    for c, *_ in ch:
        off.append(len(allpts))
        allpts += c.points
    for j, (c, b, dr, *_r) in enumerate(ch):
        for f, (k, d, P), sl, (_, _, v, fv), vm in ((2 * j, c.kf1, c.slots1, b.k1, v1), (2 * j + 1, c.kf2, c.slots2, b.k2, v2)):
            m = len(k)
            n[f] = m; kp[f, :m] = k; ds[f, :m] = d; poses[f] = P; vm[j, :m] = v
            slots[f, :m] = np.where(sl >= 0, sl + off[j], -1)
            nfv[f] = len(fv[0]); fn[f, :len(fv[0])] = fv[0]; fs[f, :len(fv[1])] = fv[1]; ff[f, :m] = fv[2]
        draws[j] = dr
    pts, pd, pb, _, _ = LC.FC.table_arrays(allpts)
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    Tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dk, dd, dn = Tt(kp.view(np.uint8).reshape(nf, cap, 28)), Tt(ds), Tt(n)
    f1, f2 = Tt(np.arange(0, nf, 2, dtype=np.int32)), Tt(np.arange(1, nf, 2, dtype=np.int32))
    dpose, dslots = Tt(poses.view(np.uint8)), Tt(slots)
    dpts, dpd, dpb = Tt(pts.view(np.uint8)), Tt(pd), Tt(pb)
    gs = torch.zeros((nf, 3073), dtype=torch.int32, device="cuda")
    gi = torch.zeros((nf, cap), dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_frame_grid_batch_device(h, p(dk), p(dn), nf, cap, *LC.BOUNDS, p(gs), p(gi), s))
    I32 = lambda *sh: torch.full(sh, -9, dtype=torch.int32, device="cuda")  # noqa: E731
    m12, nm = I32(B, cap), I32(B)
    ext._check(L.pgorb_search_by_bow_keyframes_batch_device(h, p(dk), p(dd), p(dn), cap, p(Tt(fn.view(np.int32))), p(Tt(fs)), p(Tt(ff.view(np.int32))),
                                                            p(Tt(nfv)), p(f1), p(f2), B, p(Tt(v1)), p(Tt(v2)), LC.NNRATIO, 1, p(m12), p(nm), s))
    # (entries of d_matches12 past a key frame's n are never read by the solver)
    out = pg.Sim3Solver.iterate_batch_device(ext, dk, dn, cap, f1, f2, dpose, dslots, m12, len(allpts), dpts, dpb, Tt(draws.view(np.int32)),
                                             0.99, 20, 300, 300)
    s12, nfound = I32(B, cap), I32(B)
    ext._check(L.pgorb_search_by_sim3_batch_device(h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(f1), p(f2), B, p(dpose), *LC.BOUNDS, p(dslots),
                                                   len(allpts), p(dpts), p(dpd), p(dpb), p(out["found_sim3"]), p(out["already1"]), p(out["already2"]),
                                                   SC.CHAIN_TH, p(s12), p(nfound), s))
    torch.cuda.synchronize()                                             # the first download
    H = lambda t: t.cpu().numpy()  # noqa: E731
    found = np.frombuffer(H(out["found"]).tobytes(), SIM3_ESTIMATE_DTYPE)
    best = np.frombuffer(H(out["best"]).tobytes(), SIM3_ESTIMATE_DTYPE)
    sim3 = np.frombuffer(H(out["found_sim3"]).tobytes(), SIM3_DTYPE)
    for j, (c, b, dr, rm12, sc, r, (n3, rs12)) in enumerate(ch):
        a, b2 = len(c.slots1), len(c.slots2)
        assert int(nm[j]) == int((rm12 >= 0).sum()) and np.array_equal(H(m12[j, :a]), rm12), "%s: SearchByBoW" % c.name
        got = SC.result_of(H(out["ninliers"])[j], found[j], sim3[j], best[j], H(out["inlier"][j, :a]), H(out["matches12_out"][j, :a]),
                           H(out["already1"][j, :a]), H(out["already2"][j, :b2]), H(out["info"][j]))
        _check(sc, r, got, "chained", SC.spread(sc))
        # the third stage's reference reads the transform the device produced, which the second stage has just compared
        kf1, kf2 = c.build()
        import loop_reference as LR
        w3 = LR.search_by_sim3(kf1, kf2, sim3[j], list(got["already1"]), list(got["already2"]), c.th)
        assert int(nfound[j]) == w3[0] and np.array_equal(H(s12[j, :a]), np.array(w3[1], np.int32)), "%s: SearchBySim3" % c.name
        assert w3[0] == n3 and np.array_equal(np.array(w3[1], np.int32), rs12), "%s: ... and the all-reference chain finds the same" % c.name


# ---------------------------------------------------------------- the C++ mirror (pilotguru_amd/host/orb_extractor.hpp)
CPP_DRIVER = r"""
// reads problems written by tests/test_sim3_solver.py and prints what pgorb::Sim3Solver::iterate returns: "ok nInliers bNoMore
// mnIterations mnBestInliers", then found | foundSim3 | best | vbInliers | matches12Out | already1 | already2 as hex bytes, or the exception
#include <cstdio>
#include <cstring>
#include <fstream>
#include "pilotguru_amd/host/orb_extractor.hpp"
using namespace pgorb;
template <class T> static void rd(std::ifstream& f, std::vector<T>& v) { int32_t n; f.read((char*)&n, 4); v.resize(n); if (n) f.read((char*)v.data(), (size_t)n * sizeof(T)); }
static void hex(const void* p, size_t n) { for (size_t i = 0; i < n; i++) std::printf("%02x", ((const unsigned char*)p)[i]); }
int main(int argc, char** argv)
{
    const bool run = argc > 1 && std::strcmp(argv[1], "run") == 0;        // "check": no context, the mirror's checks only
    ORBextractor* ext = run ? new ORBextractor(1000, 1.2f, 8, 20, 7, 640, 480) : nullptr;
    for (int a = 2; a < argc; a++) {
        std::ifstream f(argv[a], std::ios::binary);
        Frame F1, F2; pgorb_kf_pose pose1, pose2; std::vector<int32_t> s1, s2, m12; std::vector<pgorb_map_point> points; std::vector<uint8_t> bad;
        std::vector<uint32_t> draws; pgorb_sim3_params prm;
        rd(f, F1.mvKeysUndistorted); rd(f, F2.mvKeysUndistorted); f.read((char*)&pose1, sizeof pose1); f.read((char*)&pose2, sizeof pose2);
        rd(f, s1); rd(f, s2); rd(f, m12); rd(f, points); rd(f, bad); rd(f, draws); f.read((char*)&prm, sizeof prm);
        try {
            Sim3Solver S(ext ? ext->context() : nullptr, F1, F2, pose1, pose2, s1, s2, m12, points, bad, draws, prm.fix_scale != 0);
            S.SetRansacParameters(prm.probability, prm.min_inliers, prm.max_iterations);
            S.mnIterations = prm.first_iteration; S.mnBestInliers = prm.best_inliers_in;
            bool noMore; std::vector<bool> inl; int n;
            const bool ok = S.iterate(prm.niterations, noMore, inl, n);
            std::printf("%d %d %d %d %d\n", ok ? 1 : 0, n, noMore ? 1 : 0, S.mnIterations, S.mnBestInliers);
            hex(&S.found, sizeof S.found); hex(&S.foundSim3, sizeof S.foundSim3); hex(&S.best, sizeof S.best);
            for (size_t i = 0; i < inl.size(); i++) std::printf("%02x", inl[i] ? 1 : 0);
            hex(S.matches12Out.data(), S.matches12Out.size() * 4); hex(S.already1.data(), S.already1.size()); hex(S.already2.data(), S.already2.size());
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
    src, exe = os.path.join(str(tmp_path), "sim3_driver.cc"), os.path.join(str(tmp_path), "sim3_driver")
    open(src, "w").write(CPP_DRIVER)
    lib = os.path.join(root, "pilotguru_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", root, src, "-o", exe, "-L", lib, "-lpgorb", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _write_problem(path, c, **prm):
    def arr(a, dt):
        a = np.ascontiguousarray(a, dt)
        return np.int32(a.shape[0]).tobytes() + a.tobytes()
    k1, k2, pts = SC.keypoints(c.octaves1)[:c.n1], SC.keypoints(c.octaves2)[:c.n2], SC.table(c.points)[:len(c.points)]
    with open(path, "wb") as f:
        f.write(arr(k1, k1.dtype) + arr(k2, k2.dtype) + np.asarray(SC.pose_record(c.pose1)).tobytes() + np.asarray(SC.pose_record(c.pose2)).tobytes() +
                arr(c.kf_point1, np.int32) + arr(c.kf_point2, np.int32) + arr(c.matches12, np.int32) + arr(pts, pts.dtype) +
                arr(np.zeros(0, np.uint8) if c.bad is None else c.bad, np.uint8) + arr(c.draws.reshape(-1), np.uint32) +
                SC.params_record(dict(c.params, **prm)).tobytes())


def _run_driver(exe, mode, paths):
    import subprocess
    return subprocess.run([exe, mode] + paths, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines()


def test_cpp_mirror_rejects_bad_inputs_before_calling_the_library(tmp_path):
    """pgorb::Sim3Solver throws std::invalid_argument for every input pgorb_sim3_solver would refuse, before any pointer reaches
    the library; well-formed input reaches it (a NULL context here, so PGORB_E_ARG comes back as std::runtime_error)."""
    exe = _cpp_driver(tmp_path)
    c = cases()["sparse_slots"]
    bad = [(w, v, {}) for w, v in _bad_arrays(c)[0]] + [("matches12 too short", c.variant(matches12=c.matches12[:-1]), {})] + \
        [(repr(p), c, p) for p in BAD_PARAMS] + [("max_iterations 1025", c, dict(max_iterations=1025))]
    paths = [os.path.join(str(tmp_path), "p%d.bin" % i) for i in range(len(bad) + 1)]
    _write_problem(paths[0], c)
    for path, (_, v, prm) in zip(paths[1:], bad):
        _write_problem(path, v, **prm)
    out = _run_driver(exe, "check", paths)
    assert out[0] == "runtime_error"
    assert out[1:] == ["invalid_argument"] * len(bad), [w for (w, _, _), o in zip(bad, out[1:]) if o != "invalid_argument"]


@pytest.mark.gpu
def test_gpu_cpp_mirror_equals_the_single_call(ext, tmp_path):
    exe = _cpp_driver(tmp_path)
    names = ["sparse_slots", "resume_carried_best", "heavy_outliers", "few_19", "scale_fixed_unit"]
    c = cases()["sparse_slots"]
    o1 = c.octaves1.copy()
    o1[_bad_arrays(c)[1][0]] = SC.NLEVELS
    paths = [os.path.join(str(tmp_path), "%s.bin" % n) for n in names + ["octave"]]
    for n, path in zip(names, paths):
        _write_problem(path, cases()[n])
    _write_problem(paths[-1], c.variant(octaves1=o1))
    out = _run_driver(exe, "run", paths)
    assert out[-1] == "invalid_argument"
    for i, n in enumerate(names):
        g = SC.run_gpu(cases()[n], ext)
        head, body = out[2 * i], out[2 * i + 1]
        assert [int(x) for x in head.split()] == [int(bool(g["status"] & SR.S3_FOUND)), g["ret"], int(bool(g["status"] & (SR.S3_FEW | SR.S3_NO_MORE))),
                                                  g["its_after"], g["best_inliers"]], n
        raw = g["raw"][:-28]                                            # (without the info words)
        assert bytes.fromhex(body) == raw, n
