"""pgorb_local_bundle_adjustment (pilotguru_amd/csrc/local_ba.hip): Optimizer::LocalBundleAdjustment on the GPU against the plain
reference of tests/lba_reference.py on the constructed windows of tests/lba_cases.py.

The CPU tests anchor the reference's reading of g2o (the analytic Jacobians against central differences, one Schur solve against
numpy.linalg.solve on the full damped system, a noise-free scene, the exact optimum, the set derivation against a literal
transcription), hold every case to the case condition under every arithmetic form, show what each rule mutant changes, and keep
tests/golden/lba_spread.json up to date.  The GPU tests compare the single call and the batched form with the reference (integers
exactly, floats by lba_cases.bounds), the batch with its singles byte for byte, a window alone, first, last, on a second stream and
repeated, the chain into pgorb_refresh_map_points_batch_device, the refusals and the capacities.

On the MI355X every integer and every float output of every case equalled the reference's bit for bit (the recorded spread between
the reference's forms is below one float ulp everywhere, so the bound is 2 float ulps)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import lba_cases as LC  # noqa: E402
import lba_reference as LR  # noqa: E402
import map_point_reference as MR  # noqa: E402
import pose_reference as PR  # noqa: E402

f32, f64 = np.float32, np.float64
NAMES = ("pgorb_local_bundle_adjustment", "pgorb_local_bundle_adjustment_batch_device")
# mutants that cannot change an output; test_equivalent_mutants_change_nothing_and_why shows why
EQUIVALENT = ("errors_recomputed_after_reject", "inactive_vertex_kept")


# ---------------------------------------------------------------- presence
def test_symbols_and_mirrors_are_present():
    """The two entry points are exported and refuse a NULL context; both mirrors and the constants exist and agree with the header."""
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    z = np.zeros(64, f32)
    p = C.c_void_p(z.ctypes.data)
    assert L.pgorb_local_bundle_adjustment(None, 0, p, p, p, None, p, None, 0, p, 0, p, None, p, p, p, 2, p, p, p, p, p, p, None) == _lib.PGORB_E_ARG
    assert L.pgorb_local_bundle_adjustment_batch_device(None, p, p, 0, 1, p, None, p, None, p, p, 0, 0, 0, p, None, p, p, p, 0, 2, p, p, p, p, p, p,
                                                        None, None, None) == _lib.PGORB_E_ARG
    assert (pg.LBA_NOTHING, pg.LBA_NONFINITE, pg.LBA_INFO) == (LR.LBA_NOTHING, LR.LBA_NONFINITE, LR.INFO)
    assert (pg.LBA_MAX_LOCAL_KF, pg.LBA_MAX_FIXED_KF, pg.LBA_MAX_POINTS, pg.LBA_MAX_EDGES) == (LR.MAX_LOCAL_KF, LR.MAX_FIXED_KF, LR.MAX_POINTS, LR.MAX_EDGES)
    assert callable(pg.Optimizer.LocalBundleAdjustment) and callable(pg.Optimizer.LocalBundleAdjustment_batch_device)
    hpp = open(os.path.join(ROOT, "pilotguru_amd", "host", "orb_extractor.hpp")).read()
    assert "LocalBundleAdjustmentResult LocalBundleAdjustment(" in hpp and "pgorb_local_bundle_adjustment(ctx_" in hpp
    hdr = open(os.path.join(ROOT, "include", "pgorb.h")).read()
    assert all(("int  %s(" % n) in hdr for n in NAMES)
    for text in ("#define PGORB_LBA_INFO           10", "#define PGORB_LBA_MAX_LOCAL_KF   64", "#define PGORB_LBA_MAX_FIXED_KF   256",
                 "#define PGORB_LBA_MAX_POINTS     8192", "#define PGORB_LBA_MAX_EDGES      65536", "#define PGORB_LBA_LIMIT          4"):
        assert text in hdr, text


def test_cpp_mirror_compiles():
    """host/orb_extractor.hpp with the new mirror is valid C++17 (syntax only: no device is needed)."""
    src = "#include \"orb_extractor.hpp\"\nint main() { pgorb::Optimizer o(nullptr); (void)o; return 0; }\n"
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                        os.path.join(ROOT, "pilotguru_amd", "host"), "-x", "c++", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]


# ---------------------------------------------------------------- anchors of the reading
def _graph(name, rules=LR.REFERENCE):
    P, _ = LC.case(name)
    is_local, role, edge = LR.derive_sets(P, rules)
    G = LR.build_graph(P, is_local, role, edge, rules, LR.Form())
    q, t = np.zeros((P.nframes, 4)), np.zeros((P.nframes, 3))
    q[:, 3] = 1.0
    for f in range(P.nframes):
        if role[f]:
            E = PR.to_se3(P.Tcw[f])
            q[f], t[f] = E.q, E.t
    return P, G, q, t, P.pos[G.pts].astype(f64)


def test_analytic_jacobians_equal_central_differences_of_the_reference_error():
    """EdgeSE3ProjectXYZ::linearizeOplus against central differences of the reference's own computeError under its own oplus
    (exp(update) * estimate for the camera, += for the point).  With step h the difference carries h^2 times a third derivative
    (of the order of the Jacobian itself here) and the rounding of two errors of magnitude 1e3 pixels over 2h."""
    P, G, q, t, X = _graph("structure")
    sel = np.arange(len(G.k))
    pc, _, _ = LR.project(q, t, X, G, sel)
    Ji, Jj = LR.jacobians(q, pc, G, sel)
    h = 1e-6
    worst = 0.0
    for e in sel[::3]:
        f, p = G.frame[e], G.pt[e]
        bound = 10.0 * (h * h * max(1.0, np.abs(Jj[e]).max(), np.abs(Ji[e]).max()) + np.finfo(f64).eps * 1e3 / h)
        for k in range(6):
            err = []
            for s in (+h, -h):
                u = np.zeros(6)
                u[k] = s
                E = PR.oplus(PR.SE3(q[f], t[f]), u)
                q2, t2 = q.copy(), t.copy()
                q2[f], t2[f] = E.q, E.t
                _, e0, e1 = LR.project(q2, t2, X, G, np.array([e]))
                err.append(np.array([e0[0], e1[0]]))
            d = np.abs((err[0] - err[1]) / (2 * h) - Jj[e][:, k]).max()
            worst = max(worst, d / bound)
            assert d <= bound, (e, k, d, bound)
        for k in range(3):
            err = []
            for s in (+h, -h):
                X2 = X.copy()
                X2[p, k] += s
                _, e0, e1 = LR.project(q, t, X2, G, np.array([e]))
                err.append(np.array([e0[0], e1[0]]))
            d = np.abs((err[0] - err[1]) / (2 * h) - Ji[e][:, k]).max()
            assert d <= bound, (e, k, d, bound)
    assert worst > 0.0


def test_one_schur_solve_equals_the_full_damped_system():
    """BlockSolver::solve's Schur complement, reduced Cholesky and back-substitution against numpy.linalg.solve on the full
    (6 nl + 3 np) system with lambda on every diagonal entry, under both factorisations."""
    for name in ("kf2", "kf11", "no_gauge"):
        P, G, q, t, X = _graph(name)
        S = LR.State()
        S.q, S.t, S.X, S.err = q, t, X, np.zeros((len(G.k), 2))
        act = np.arange(len(G.k))
        _, Hpp, bp, Hll, bl, W, col, p = LR.linear_system(S, G, act, True, LR.Form())
        nc, npt, lam = len(Hpp), len(Hll), 3.7
        n = 6 * nc + 3 * npt
        H, b = np.zeros((n, n)), np.concatenate([bp.reshape(-1), bl.reshape(-1)])
        for c in range(nc):
            H[6 * c:6 * c + 6, 6 * c:6 * c + 6] = Hpp[c]
        for j in range(npt):
            H[6 * nc + 3 * j:6 * nc + 3 * j + 3, 6 * nc + 3 * j:6 * nc + 3 * j + 3] = Hll[j]
        for e in np.flatnonzero(col >= 0):
            r, c = slice(6 * col[e], 6 * col[e] + 6), slice(6 * nc + 3 * p[e], 6 * nc + 3 * p[e] + 3)
            H[r, c] += W[e]
            H[c, r] += W[e].T
        want = np.linalg.solve(H + lam * np.eye(n), b)
        for chol in ("llt", "ldlt"):
            ok, xp, xl = LR.schur_solve(Hpp, bp, Hll, bl, W, col, p, lam, lam, np.ones(nc, bool), np.ones(npt, bool), LR.Form(chol=chol), {})
            got = np.concatenate([xp.reshape(-1), xl.reshape(-1)])
            assert ok and np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (name, chol)


def test_noise_free_scene_returns_the_generating_poses_and_points():
    """Two fixed cameras hold the gauge; started off the truth without noise, the result is what generated the observations up to
    the float rounding of the keypoints and of the fixed poses (1e-7 of 500 pixels at 6 m is 1e-6 m)."""
    P = LC.window("anchor", 901, 3, 2, 30, nobs=4, noise=0.0, far=0, twist=(0.01, 0.05))
    r = LR.local_bundle_adjustment(P, 2)
    assert r["info"][0] == 0 and r["ret"] == 0
    for f in np.flatnonzero(r["role"] == LR.ROLE_LOCAL):
        T = r["pose_Tcw"][f].reshape(3, 4).astype(f64)
        assert np.abs(T[:, :3] - P.true_T[f][:, :3]).max() < 5e-6 and np.abs(T[:, 3] - P.true_T[f][:, 3]).max() < 5e-5, f
        assert np.abs(P.Tcw[f].reshape(3, 4)[:, 3] - P.true_T[f][:, 3]).max() > 1e-3          # it did start off the truth
    loc = np.flatnonzero(r["is_local"])
    assert np.abs(r["pos"][loc] - P.true_X[loc]).max() < 2e-4 and float(r["chi2"].max()) < 1e-4


def test_exact_optimum_takes_the_rho_zero_path_and_changes_nothing():
    """Started at a binary-exact optimum b is 0, the update is 0, tempChi == currentChi, rho == 0: the trial is rejected (pop) and
    the iteration returns Terminate, in both optimize calls.  Points and translations come back bit for bit."""
    P, rounds = LC.case("exact_optimum")
    r = LC.run_reference("exact_optimum")
    assert list(r["info"][5:9]) == [1, 1, 1, 1] and r["hits"]["terminate"] == 2 and r["hits"]["round1_ended_rejected"] == 1
    assert r["ret"] == 0 and not r["chi2"].any() and r["pos"].tobytes() == P.pos.tobytes()
    for f in np.flatnonzero(r["role"] == LR.ROLE_LOCAL):
        assert r["pose_Tcw"][f].tobytes() == P.Tcw[f].tobytes()


def test_set_derivation_equals_the_literal_transcription():
    """The flags against Optimizer.cc:455-504 written out with its lists and mnBALocalForKF / mnBAFixedForKF marks, as sets."""
    for name in LC.CASE_NAMES:
        P, _ = LC.case(name)
        is_local, role, edge = LR.derive_sets(P)
        lkf, lmp, lfix, ledges = LR.literal_sets(P)
        assert set(np.flatnonzero(role == LR.ROLE_LOCAL)) == lkf, name
        assert set(np.flatnonzero(is_local)) == lmp and set(np.flatnonzero(role == LR.ROLE_FIXED)) == lfix, name
        pt_of = np.repeat(np.arange(len(P.pos)), np.diff(P.obs_start))
        assert {(int(pt_of[k]), int(P.obs_frame[k])) for k in np.flatnonzero(edge)} == ledges, name
    P, _ = LC.case("structure")
    is_local, role, edge = LR.derive_sets(P)
    assert P.kf_bad[P.local_kf].any() and P.point_bad.any() and (P.kf_bad[P.obs_frame] == 1).any()       # the case holds what it claims


# ---------------------------------------------------------------- the cases
def test_cases_hold_what_they_claim():
    info = {n: LC.run_reference(n) for n in LC.CASE_NAMES}
    assert [int(info[n]["info"][3]) for n in ("kf1", "kf2", "kf10", "kf11")] == [1, 2, 10, 11]
    assert [int(info["edges%d" % n]["info"][1]) for n in (63, 64, 65, 257)] == [63, 64, 65, 257]
    assert int(info["points257"]["info"][2]) == 257
    assert int(info["no_gauge"]["info"][4]) == 0 and not LC.case("no_gauge")[0].fixed_id0.any()
    P = LC.case("id0_local")[0]
    assert P.fixed_id0[P.local_kf].any()
    r = info["structure"]
    P = LC.case("structure")[0]
    lens = np.diff(P.obs_start)
    pt_of = np.repeat(np.arange(len(P.pos)), lens)
    assert ((lens == 1) & (r["is_local"] == 1)).any()                                                  # a point seen once
    assert any(r["level"][P.obs_start[p]:P.obs_start[p + 1]].all() and lens[p] >= 2 for p in np.flatnonzero(r["is_local"]))
    lost = [f for f in np.flatnonzero(r["role"] == LR.ROLE_LOCAL) if (P.obs_frame == f).any() and r["level"][(P.obs_frame == f) & (r["is_local"][pt_of] == 1)].all()]
    assert lost, "no local key frame lost all its level-0 edges"
    assert len(set(map(tuple, P.cam))) == 2 and set(np.concatenate(P.octaves)) == set(range(LC.NLEVELS))
    assert info["outliers"]["info"][9] >= 20 and info["rounds1"]["info"][7] == 0 and info["rounds1"]["info"][9] == 0
    assert info["depth_survivor"]["hits"]["set_aside_for_depth_alone"] == 1 and info["depth_survivor"]["hits"]["depth_only_survivor"] == 1
    assert info["exact_optimum"]["hits"]["round1_ended_rejected"] == 1
    assert any(info[n]["hits"].get("stopped_by_1e3") for n in LC.CASE_NAMES)


def test_spread_file_is_up_to_date():
    """tests/golden/lba_spread.json (tests/golden/make_lba_spread.py writes it) holds what the reference shows now."""
    rec = LC.recorded_spread()
    assert sorted(rec) == sorted(LC.CASE_NAMES)
    for n in LC.CASE_NAMES:
        now = LC.spread(n)
        assert sorted(now) == sorted(rec[n]), n
        for k in now:
            assert abs(now[k] - rec[n][k]) <= 1e-3 * max(now[k], rec[n][k]) + 1e-300, (n, k, now[k], rec[n][k])


def test_every_case_meets_the_case_condition_under_every_form():
    """No chi2 at a classification near 5.991, no depth near 0, no Levenberg decision near its threshold, and the same integers
    under all twelve arithmetic forms: the reference alone shows that the exact comparisons are safe."""
    rec = LC.recorded_spread()
    bad = [b for n in LC.CASE_NAMES for b in LC.condition(n, rec[n])]
    assert bad == [], bad[:5]


def _changed(rules):
    rec = LC.recorded_spread()
    return [n for n in LC.CASE_NAMES if LC.differences(LC.case(n)[0], LC.run_reference(n), LC.run_reference(n, rules=rules), rec[n])]


def test_every_mutant_changes_a_compared_output():
    for m, rules in LR.MUTANTS.items():
        if m not in EQUIVALENT:
            assert _changed(rules), m
    assert "depth_survivor" in _changed(LR.MUTANTS["depth_on_stale_estimates"])
    assert "id0_local" in _changed(LR.MUTANTS["id0_not_fixed"]) and "structure" in _changed(LR.MUTANTS["lambda_init_over_poses_only"])


def test_equivalent_mutants_change_nothing_and_why():
    """Two readings leave no trace in a compared output on finite data.  (6) An optimize call can end on a rejected trial only after
    ten rejections in a row -- lambda has then grown by 2^55, so the rejected state differs from the estimate by a step of about
    b / (2^55 lambda): not zero in double, but far below the float the chi2 is rounded to and below the case condition's window -- or
    with rho == 0, where the update is 0.  The constructed cases hold only the second kind (exact_optimum); no case ends an optimize
    on ten rejections, so the device's read of a stored error that differs from the estimate's is exercised inside the trial loop
    only.  Not equivalent in the strict sense: a rejected last trial whose chi2 is NaN leaves NaN stored errors, which the reference
    (and the library) report as LBA_NONFINITE and the mutant would not.  (8) A vertex without a level-0 edge has a zero gradient and no coupling:
    kept active, its block is lambda * I, its update exactly 0, and computeLambdaInit and computeScale see zeros."""
    for m in EQUIVALENT:
        assert _changed(LR.MUTANTS[m]) == [], m
    P, G, q, t, X = _graph("structure")
    S = LR.State()
    S.q, S.t, S.X, S.err = q, t, X, np.zeros((len(G.k), 2))
    r = LC.run_reference("structure")
    level = r["level"][G.k]
    act = np.flatnonzero(level == 0)
    _, Hpp, bp, Hll, bl, W, col, p = LR.linear_system(S, G, act, False, LR.Form())
    idle = [c for c in range(len(Hpp)) if not (col == c).any()]
    assert idle, "the case has a camera without a level-0 edge"
    ok, xp, xl = LR.schur_solve(Hpp, bp, Hll, bl, W, col, p, 2.5, 2.5, np.ones(len(Hpp), bool), np.ones(len(Hll), bool), LR.Form(), {})
    assert ok and all(not xp[c].any() and not Hpp[c].any() for c in idle)
    idle_pts = [j for j in range(len(Hll)) if not (p == j).any()]
    assert idle_pts and all(not xl[j].any() for j in idle_pts)


def test_mirror_refuses_malformed_input_without_a_device():
    """Optimizer.LocalBundleAdjustment raises ValueError for what the library's checked call refuses, before the library is called."""
    import pilotguru_amd as pg

    class Ext:
        def GetLevels(self):
            return LC.NLEVELS

    class KF:
        pass
    P, _ = LC.case("kf2")

    def call(**kw):
        kfs = []
        for f in range(P.nframes):
            k = KF()
            k.N, k.mvKeysUndistorted = len(P.octaves[f]), LC.keypoints(P.keys_xy[f], P.octaves[f])
            kfs.append(k)
        a = dict(key_frames=kfs, poses=LC.pose_records(P), kf_point=[s.copy() for s in P.kf_point], local_kf=P.local_kf, points=LC.table(P),
                 obs_start=P.obs_start, obs_frame=P.obs_frame.copy(), obs_idx=P.obs_idx.copy(), rounds=2, ext=Ext())
        a.update(kw)
        return pg.Optimizer.LocalBundleAdjustment(**a)
    bad_pose, bad_fx, bad_pts, bad_oct = LC.pose_records(P), LC.pose_records(P), LC.table(P), None
    bad_pose["Tcw"][1, 3] = np.nan
    bad_fx["fx"][0] = 0.0
    bad_pts["pos"][2, 1] = np.inf
    slots = [s.copy() for s in P.kf_point]
    slots[0][0] = len(P.pos)
    twice = P.obs_frame.copy()
    twice[1] = twice[0]
    far = P.obs_idx.copy()
    far[0] = 10 ** 6
    for what, kw in (("rounds", dict(rounds=3)), ("pose", dict(poses=bad_pose)), ("fx", dict(poses=bad_fx)), ("point", dict(points=bad_pts)),
                     ("slot", dict(kf_point=slots)), ("local", dict(local_kf=[0, P.nframes])), ("start", dict(obs_start=P.obs_start[::-1].copy())),
                     ("twice", dict(obs_frame=twice)), ("idx", dict(obs_idx=far))):
        with pytest.raises(ValueError):
            call(**kw)
            pytest.fail(what)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(1000, 1.2, LC.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=4)
    assert np.array_equal(np.asarray(e.GetInverseScaleSigmaSquares(), f32)[:LC.NLEVELS], LC.INV_SIGMA2)
    yield e
    e.close()


def _check(name, want, got, what):
    P, _ = LC.case(name)
    assert not isinstance(got, int), "%s (%s): error %r" % (name, what, got)
    rec = LC.recorded_spread()[name]
    d = LC.scaled_differences(P, want, got)
    print("%s (%s): " % (name, what) + ", ".join("%s %.2g / %.2g" % (k, d[k], LC.bounds(rec)[k]) for k in LC.FLOAT_OUTPUTS))
    assert LC.differences(P, want, got, rec) == [], "%s (%s)" % (name, what)
    assert got["other_bytes"] == LC.other_bytes(LC.table(P)), "%s: normal and distances keep their bytes" % name
    if what == "single":                                        # pose_out of a key frame that is not local: the input, copied
        assert got["pose_rest_bytes"] == got["pose_in_rest_bytes"], "%s: pose_out of the other key frames is the input" % name
    elif what == "batch":                                       # the batched form leaves those records alone
        assert set(got["pose_rest_bytes"]) <= {LC.POSE_SENTINEL}, "%s: pose_out is written for local key frames only" % name
    notloc = np.flatnonzero(got["is_local"] == 0)
    assert got["pos"][notloc].tobytes() == P.pos[notloc].tobytes(), "%s: only local points move" % name


@pytest.mark.gpu
@pytest.mark.parametrize("name", LC.CASE_NAMES)
def test_gpu_single_call_equals_the_reference(ext, name):
    P, rounds = LC.case(name)
    _check(name, LC.run_reference(name), LC.run_gpu(P, rounds, ext), "single")


@pytest.fixture(scope="module")
def singles(ext):
    return {n: LC.run_gpu(LC.case(n)[0], LC.case(n)[1], ext) for n in LC.CASE_NAMES}


BYTES = ("ret", "erase", "chi2", "level", "is_local", "role", "info", "pose_bytes", "table_bytes")
BATCH = [n for n in LC.CASE_NAMES if n != "rounds1"]          # one `rounds` a call


def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in BYTES)


@pytest.mark.gpu
def test_gpu_batch_equals_the_reference_and_its_singles_byte_for_byte(ext, singles):
    """Windows of different sizes over one batch whose cap_per_frame is no multiple of 64."""
    b = LC.Batch(BATCH)
    assert b.cap % 64
    got = LC.run_gpu_batch(b, ext)
    for n, r in zip(BATCH, got):
        _check(n, LC.run_reference(n), r, "batch")
        assert _same(singles[n], r) and r["elsewhere_zero"], n
    one = LC.run_gpu_batch(LC.Batch(["rounds1"]), ext)[0]
    assert _same(singles["rounds1"], one)


@pytest.mark.gpu
def test_gpu_window_is_the_same_alone_first_last_on_a_second_stream_and_repeated(ext, singles):
    import torch
    names = ["kf10", "outliers", "structure", "points257"]
    b = LC.Batch(names)
    base = LC.run_gpu_batch(b, ext)
    for order, stream in (([0], None), ([0, 1, 2, 3], None), ([3, 2, 1, 0], None), ([2, 0, 3, 1], torch.cuda.Stream()), ([0, 1, 2, 3], None)):
        got = LC.run_gpu_batch(b, ext, order, stream)
        for j, r in zip(order, got):
            assert _same(base[j], r) and _same(singles[names[j]], r), (names[j], order)


@pytest.mark.gpu
def test_gpu_chain_into_the_map_point_refresh_on_resident_arrays(ext):
    """LBA -> pgorb_refresh_map_points_batch_device (normal and depth, select = the local points) with nothing downloaded in between,
    against the reference's SetWorldPos followed by UpdateNormalAndDepth (tests/map_point_reference.py)."""
    names = ["kf10", "outliers"]
    b = LC.Batch(names)
    ref_obs = [np.zeros(len(P.pos), np.int32) for P in b.problems]
    got, tb = LC.run_gpu_batch(b, ext, refresh=ref_obs)
    sf = np.asarray(ext.GetScaleFactors(), f32)
    for j, (n, r) in enumerate(zip(names, got)):
        P = b.problems[j]
        want = LC.run_reference(n)
        _check(n, want, dict(r, other_bytes=LC.other_bytes(LC.table(P))), "chain")
        rows = tb[int(b.p0[j]):int(b.p0[j + 1])]
        kfs = [MR.KeyFrame(LC.keypoints(P.keys_xy[f], P.octaves[f]), np.zeros((len(P.octaves[f]), 32), np.uint8),
                           r["pose_Ow"][f] if r["role"][f] == LR.ROLE_LOCAL else PR.to_pose_floats(PR.to_se3(P.Tcw[f]))[1]) for f in range(P.nframes)]
        # the adjustment is held to the reference above (within the bounds); the refresh is exact on the floats the adjustment left
        for p in np.flatnonzero(r["is_local"]):
            mp = MR.MapPoint(r["pos"][p], np.zeros(32, np.uint8))
            mp.obs = [(kfs[P.obs_frame[k]], int(P.obs_idx[k])) for k in range(P.obs_start[p], P.obs_start[p + 1])]
            if not mp.obs:
                continue
            mp.ref = mp.obs[0][0]
            assert MR.update_normal_and_depth(mp, sf, LC.NLEVELS)
            assert rows["normal"][p].tobytes() == mp.normal.tobytes() and f32(rows["min_distance"][p]) == mp.min_d and \
                f32(rows["max_distance"][p]) == mp.max_d, (n, p)
        for p in np.flatnonzero(r["is_local"] == 0):
            assert rows[p].tobytes() == np.asarray(LC.table(P))[p].tobytes()


@pytest.mark.gpu
def test_gpu_python_mirror_equals_the_single_call(ext, singles):
    import pilotguru_amd as pg

    class KF:
        pass
    for name in ("structure", "outliers", "rounds1"):
        P, rounds = LC.case(name)
        kfs = []
        for f in range(P.nframes):
            k = KF()
            k.ext, k.N, k.mvKeysUndistorted = ext, len(P.octaves[f]), LC.keypoints(P.keys_xy[f], P.octaves[f])
            kfs.append(k)
        r = pg.Optimizer.LocalBundleAdjustment(kfs, LC.pose_records(P), P.kf_point, P.local_kf, LC.table(P), P.obs_start, P.obs_frame, P.obs_idx,
                                               P.point_bad, P.kf_bad, P.fixed_id0, rounds)
        s = singles[name]
        assert r["ret"] == s["ret"] and r["points"].tobytes() == s["table_bytes"] and r["erase"].tobytes() == s["erase"].tobytes()
        assert r["chi2"].tobytes() == s["chi2"].tobytes() and r["level"].tobytes() == s["level"].tobytes() and r["status"] == s["info"][0]
        assert r["poses"][s["role"] == LR.ROLE_LOCAL].tobytes() == s["pose_bytes"]
        pt_of = np.repeat(np.arange(len(P.pos)), np.diff(P.obs_start))
        assert r["to_erase"] == [(int(P.obs_frame[k]), int(pt_of[k])) for k in np.flatnonzero(s["erase"])] and len(r["to_erase"]) == r["ret"]


def _variant(P, **kw):
    a = dict(keys_xy=P.keys_xy, octaves=P.octaves, Tcw=P.Tcw, cam=P.cam, kf_bad=P.kf_bad, kf_point=P.kf_point, fixed_id0=P.fixed_id0,
             local_kf=P.local_kf, pos=P.pos, point_bad=P.point_bad, obs_start=P.obs_start, obs_frame=P.obs_frame, obs_idx=P.obs_idx,
             inv_sigma2=P.inv_sigma2)
    a.update(kw)
    return LR.Problem(**a)


@pytest.mark.gpu
def test_gpu_library_refuses_malformed_input(ext):
    from pilotguru_amd import _lib
    P, _ = LC.case("kf2")
    T, cam, pos, octs = P.Tcw.copy(), P.cam.copy(), P.pos.copy(), [o.copy() for o in P.octaves]
    T[1, 5], cam[0, 1], pos[3, 0] = np.inf, 0.0, np.nan
    octs[int(P.obs_frame[0])][int(P.obs_idx[0])] = LC.NLEVELS
    slots = [s.copy() for s in P.kf_point]
    slots[1][0] = -2
    twice, far, start = P.obs_frame.copy(), P.obs_frame.copy(), P.obs_start.copy()
    twice[1], far[2], start[1] = twice[0], P.nframes, start[2] + 1
    for what, v, rounds in (("pose", _variant(P, Tcw=T), 2), ("fy", _variant(P, cam=cam), 2), ("point", _variant(P, pos=pos), 2),
                            ("octave", _variant(P, octaves=octs), 2), ("slot", _variant(P, kf_point=slots), 2), ("twice", _variant(P, obs_frame=twice), 2),
                            ("frame", _variant(P, obs_frame=far), 2), ("start", _variant(P, obs_start=start), 2),
                            ("local", _variant(P, local_kf=[0, -1]), 2), ("rounds", P, 0), ("rounds", P, 3)):
        assert LC.run_gpu(v, rounds, ext) == _lib.PGORB_E_ARG, what
    good = LC.run_gpu(P, 2, ext)
    assert not isinstance(good, int)
    # nothing to optimise: the window names no key frame that holds a live point
    none = LC.run_gpu(_variant(P, point_bad=np.ones(len(P.pos), np.uint8)), 2, ext)
    assert none["info"][0] == LR.LBA_NOTHING and none["ret"] == 0 and none["pose_bytes"] == none["pose_in_bytes"] and none["table_bytes"] == LC.table(P).tobytes()
    assert not none["erase"].any() and not none["chi2"].any() and not none["is_local"].any()
    # a point in the image plane of cameras with identity rotation and z = 0: its depth is exactly 0, the first chi2 is not finite
    P = LC.case("exact_optimum")[0]
    P2 = _variant(P)
    P2.pos = P.pos.copy()
    P2.pos[0, 2] = 0.0
    want = LR.local_bundle_adjustment(P2, 2)
    got = LC.run_gpu(P2, 2, ext)
    assert want["info"][0] == LR.LBA_NONFINITE and list(got["info"]) == list(want["info"])
    assert got["ret"] == 0 and got["table_bytes"] == LC.table(P2).tobytes() and got["pose_bytes"] == got["pose_in_bytes"]
    assert not got["chi2"].any() and not got["erase"].any() and not got["level"].any()


def _limit_case(nlocal, nfixed, npts, per_point, one_more_edge=False):
    """A cheap window of a given size: identity-rotation cameras on a grid, every point seen by `per_point` cameras (the first local).
    one_more_edge: one further fixed camera that sees point 0 alone -- one edge more, no point more."""
    rng = np.random.default_rng(nlocal * 7 + nfixed * 3 + npts)
    B = LC.Builder(5)
    for c in range(nlocal + nfixed):
        B.add_camera([(c % 20) * 0.15 - 1.5, (c // 20) * 0.15 - 1.0, 0.0], twist=(0.002, 0.01) if c < nlocal else None)
    for k in range(npts):
        p = B.add_point([rng.uniform(-1.5, 1.5), rng.uniform(-1, 1), rng.uniform(4, 9)], 0.02)
        cams = [k % nlocal] + [nlocal + (k + j) % nfixed if nfixed else (k + 1 + j) % nlocal for j in range(per_point - 1)]
        for f in dict.fromkeys(cams):
            B.observe(p, f, 0.5)
    if one_more_edge:
        B.observe(0, B.add_camera([0.05, 0.05, 0.0]), 0.5)
    return B.problem(list(range(nlocal)), None, "limit")


_limits = {}


def _limit(*args, **kw):
    key = args + tuple(sorted(kw.items()))
    if key not in _limits:
        _limits[key] = _limit_case(*args, **kw)
    return _limits[key]


@pytest.mark.gpu
@pytest.mark.parametrize("what, args, at", [("local key frames", (64, 2, 128, 2), 64), ("fixed key frames", (1, 256, 256, 2), 256)])
def test_gpu_key_frame_capacities_at_the_limit_and_one_past(ext, what, args, at):
    from pilotguru_amd import _lib
    P = _limit_case(*args)
    want = LR.local_bundle_adjustment(P, 2)
    assert int(want["info"][3 if "local" in what else 4]) == at
    got = LC.run_gpu(P, 2, ext)
    assert not isinstance(got, int), got
    zero = dict.fromkeys(LC.FLOAT_OUTPUTS, 0.0)
    assert LC.differences(P, want, got, zero) == [], what                                              # 2 float ulps, as every recorded case
    a = list(args)
    a["local" not in what] += 1
    if "fixed" in what:
        a[2] += 1
    P1 = _limit_case(*a)
    assert LC.run_gpu(P1, 2, ext) == _lib.PGORB_E_LIMIT and what in ext._L.pgorb_last_error(ext._h).decode(), what


@pytest.mark.gpu
def test_gpu_point_and_edge_capacities_at_the_limit_and_one_past(ext):
    """8192 local points seen by 8 cameras each are 65536 edges: both capacities at once, against the reference (one optimize: it
    takes the reference about 2 s; the bound is the 2 float ulps of every recorded case).  One more observation -- a ninth camera
    that sees point 0 alone -- is 65537 edges on 8192 points and is refused for the edges; one more point is refused for the points."""
    from pilotguru_amd import _lib
    P = _limit(2, 7, 8192, 8)
    want = LR.local_bundle_adjustment(P, 1)
    got = LC.run_gpu(P, 1, ext)
    assert not isinstance(got, int), got
    assert list(got["info"][:5]) == [0, 65536, 8192, 2, 7] and got["is_local"].all()
    assert LC.differences(P, want, got, dict.fromkeys(LC.FLOAT_OUTPUTS, 0.0)) == []
    last = lambda: ext._L.pgorb_last_error(ext._h).decode()
    P1 = _limit(2, 7, 8192, 8, one_more_edge=True)
    assert len(P1.obs_frame) == 65537 and len(P1.pos) == 8192
    assert LC.run_gpu(P1, 1, ext) == _lib.PGORB_E_LIMIT and "65536 edges" in last()
    assert LC.run_gpu(_limit(2, 7, 8193, 8), 1, ext) == _lib.PGORB_E_LIMIT and "8192 local points" in last()


@pytest.mark.gpu
def test_gpu_batched_form_reports_a_window_past_a_capacity_in_its_status(ext):
    """The batched form learns the counts on the device (k_lba_prepare, other code than the single call's host count): a window one
    past each capacity ends with PGORB_LBA_LIMIT, nothing optimised, its points untouched, and the window beside it is served.  The
    table of this batch is longer than 8192 points and the batch has more than 320 frames, so the 8193-point window and the window of
    330 cameras also run past the per-window lists (the records past them are dropped, never written out of bounds)."""
    import pilotguru_amd as pg
    over = {"limit65": (_limit(65, 2, 130, 2), 3, 65), "limit257": (_limit(1, 257, 257, 2), 4, 257), "limit330": (_limit(1, 330, 330, 2), 4, 330),
            "limit8193": (_limit(2, 7, 8193, 8), 2, 8193), "limit65537": (_limit(2, 7, 8192, 8, one_more_edge=True), 1, 65537)}
    for n, (P, _, _) in over.items():
        LC._cache[n] = (P, 2)
    names = ["limit65", "limit257", "kf2", "limit330", "limit8193", "limit65537"]
    b = LC.Batch(names)
    for n, P, r in zip(names, b.problems, LC.run_gpu_batch(b, ext)):
        if n == "kf2":
            assert r["info"][0] == 0 and LC.differences(P, LC.run_reference("kf2"), r, LC.recorded_spread()["kf2"]) == [] and r["elsewhere_zero"]
            continue
        _, field, count = over[n]
        assert r["info"][0] == pg.LBA_LIMIT and r["info"][field] == count and r["ret"] == 0, (n, list(r["info"]))
        assert r["table_bytes"] == LC.table(P).tobytes() and not r["erase"].any() and not r["chi2"].any() and not r["level"].any(), n
        assert list(r["info"][5:]) == [0] * 5 and r["elsewhere_zero"], n
