"""pgorb_pnp_solver (pilotguru_amd/csrc/pnp.hip): PnPsolver on the device, against the plain reference of tests/pnp_reference.py on the
relocalisation candidates of tests/pnp_cases.py.

The hypothesis stage is compared WITHOUT a tolerance: a 4-point EPnP reads four vectors of a null space of dimension 4 or more, so
its pose depends on the basis the SVD happens to produce, and the reference DEFINES that stage operation by operation
(tests/pnp_reference.py); every traced hypothesis of every case must equal it byte for byte, NaN equal to NaN.  The reference is
UNPINNED to OpenCV (2.4.9 cannot be built where the suite runs); the CPU tests anchor it independently of the reading: noise-free
scenes of 6 or more points return the generating pose, the Jacobi SVD agrees with numpy.linalg.svd on well-separated spectra,
qr_solve with numpy.linalg.lstsq, the closed form of the swap-with-back selection with the literal list, the RANSAC table of the
library's host function with a direct evaluation for every N in range.

Refine's pose gets, per case and output, the larger of 2 float ulps at the output's scale and 16 x the spread the reference shows
between its arithmetic forms (tests/golden/pnp_spread.json, written by tests/golden/make_pnp_spread.py): pnp_cases.bounds.  That
bound is what a parallel reduction of Refine's long sums would have to meet; the device as it stands sums in the reference's
sequential order (one thread per matrix entry), so the GPU tests also assert that Refine's pose equals the reference bit for bit."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pnp_cases as PC  # noqa: E402
import pnp_reference as PR  # noqa: E402

f32, f64 = np.float32, np.float64
CASE_NAMES = ["few_9", "n10_cap_one", "n11_clean", "n21_clean", "n63_outliers", "n64_outliers", "n65_outliers", "n257_outliers",
              "late_success", "heavy_best_at_cap", "heavy_nothing", "mixed_octaves", "sparse_bad_slots", "degenerate_draws",
              "second_camera", "at_cap_five_more", "resume_carried_best", "edge_of_threshold",
              "refine_exactly_min", "zero_depth"]
NEW_SYMBOLS = ["pgorb_pnp_solver", "pgorb_pnp_solver_batch_device", "pgorb_pnp_ransac"]
BATCH_CAP = 263                      # one cap_per_frame for every case: above the largest frame (257), no multiple of 64
_cache = {}


def cases():
    return {c.name: c for c in PC.all_cases()}


def want(name):
    return PC.reference(cases()[name])


def recorded():
    if "spread" not in _cache:
        _cache["spread"] = PC.recorded_spread()
    return _cache["spread"]


# ---------------------------------------------------------------- CPU
def test_symbols_and_mirror_exist():
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(HERE), "include", "pgorb.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in _lib.SYMBOLS and (s + "(") in header
    for m in ("SetRansacParameters", "iterate", "find", "iterate_batch_device"):
        assert callable(getattr(pg.PnPsolver, m))
    assert (pg.PNP_FEW, pg.PNP_FOUND, pg.PNP_NO_MORE, pg.PNP_REFINED, pg.PNP_INFO, pg.PNP_MAX_WINDOW) == (PR.FEW, PR.FOUND, PR.NO_MORE, PR.REFINED, 8, 1024)
    assert pg.PNP_PARAMS_DTYPE.itemsize == 36 and pg.PNP_HYPOTHESIS_DTYPE == PC.TRACE_DTYPE
    hpp = open(os.path.join(os.path.dirname(HERE), "pilotguru_amd", "host", "orb_extractor.hpp")).read()
    assert "class PnPsolver" in hpp


@pytest.mark.parametrize("prm", [(0.99, 10, 300, 4, 0.5), (0.99, 8, 300, 4, 0.4), (0.5, 4, 20, 4, 1.0)])
def test_ransac_table_equals_a_direct_evaluation(prm):
    from pilotguru_amd import _lib
    L = _lib.lib()
    for N in range(0, 401):
        a, b = C.c_int32(-7), C.c_int32(-7)
        assert L.pgorb_pnp_ransac(C.c_float(prm[0]), prm[1], prm[2], prm[3], C.c_float(prm[4]), N, C.byref(a), C.byref(b)) == 0
        assert (a.value, b.value) == PR.ransac(*prm, N), N
    # and the direct evaluation against the issue's figures: relocalisation's cap is at most 35; int(10.5) = 10; N == min gives 1
    R = lambda N: PR.ransac(0.99, 10, 300, 4, 0.5, N)
    assert max(R(N)[1] for N in range(0, 2000)) == 35 and R(21)[0] == 10 and R(10) == (10, 1) and R(64) == (32, 35) and R(65) == (32, 35)
    e = float(f32(10) / f32(11))
    assert R(11) == (10, math.ceil(math.log(1 - float(f32(0.99))) / math.log(1 - math.pow(e, 3))))


def test_closed_form_selection_equals_the_literal_list():
    rng = np.random.RandomState(3)
    for N in list(range(4, 12)) + [63, 64, 65, 257, 16000]:
        for _ in range(200):
            d = rng.randint(0, 2 ** 31, 4)
            assert PR.select_closed(d, N) == PR.select_literal(d, N)
        for d in ([0, 0, 0, 0], [2 ** 31 - 1] * 4, [2 ** 31 - 1, 0, 2 ** 31 - 1, 0], [0, 2 ** 31 - 1, 0, 2 ** 31 - 1]):
            got = PR.select_closed(d, N)
            assert got == PR.select_literal(d, N) and len(set(got)) == 4


def test_jacobi_svd_against_numpy():
    rng = np.random.RandomState(5)
    for (m, n) in ((3, 3), (6, 3), (6, 4), (6, 5), (12, 12)):
        for _ in range(5):
            U, _ = np.linalg.qr(rng.normal(size=(m, m)))
            V, _ = np.linalg.qr(rng.normal(size=(n, n)))
            s = np.sort(rng.uniform(1.0, 2.0, n) * 3.0 ** np.arange(n))[::-1]          # well separated
            A = (U[:, :n] * s) @ V.T
            W, Ut, Vt = PR.jacobi_svd([[A[r][c] for r in range(m)] for c in range(n)], True)
            assert np.allclose(W, s, rtol=1e-12) and list(W) == sorted(W, reverse=True)
            un, sn, vtn = np.linalg.svd(A, full_matrices=False)
            for i in range(n):                                                          # singular vectors up to a common sign
                sg = np.sign(np.dot(Ut[i], un[:, i]))
                assert np.allclose(np.array(Ut[i]) * sg, un[:, i], atol=1e-10) and np.allclose(np.array(Vt[i]) * sg, vtn[i], atol=1e-10)
            assert np.allclose((np.array(Ut).T * np.array(W)) @ np.array(Vt), A, atol=1e-10)
    W, _, _ = PR.jacobi_svd([[float("nan")] * 12 for _ in range(12)], False)              # a NaN matrix terminates
    assert all(w != w for w in W)


def test_small_solves_against_numpy():
    rng = np.random.RandomState(6)
    for nc in (3, 4, 5):
        L, rho = rng.normal(size=(6, nc)), rng.normal(size=6)
        x = PR.svd_solve(L.tolist(), rho.tolist())
        assert np.allclose(x, np.linalg.lstsq(L, rho, rcond=None)[0], atol=1e-10)
    A, b = rng.normal(size=(6, 4)), rng.normal(size=6)
    X = [9.0] * 4
    assert PR.qr_solve(A.tolist(), b.tolist(), X) and np.allclose(X, np.linalg.lstsq(A, b, rcond=None)[0], atol=1e-10)
    A[:, 0] = 0.0
    X = [9.0] * 4
    assert not PR.qr_solve(A.tolist(), b.tolist(), X) and X == [9.0] * 4                  # eta == 0: X as it was
    CC = rng.normal(size=(3, 3))
    assert np.allclose(PR.svd_invert3(CC.tolist()), np.linalg.inv(CC), atol=1e-10)


@pytest.mark.parametrize("n", [6, 7, 10, 30, 150])
def test_epnp_returns_the_generating_pose_on_noise_free_scenes(n):
    rng = np.random.RandomState(n)
    for _ in range(3):
        R, t = PC.rotation(rng.uniform(-1, 1, 3)), rng.uniform(-1, 1, 3) + np.array([0, 0, 6.0])
        X = rng.uniform(-2, 2, (n, 3))
        Xc = X @ R.T + t
        us = np.stack([PC.K1[0] * Xc[:, 0] / Xc[:, 2] + PC.K1[2], PC.K1[1] * Xc[:, 1] / Xc[:, 2] + PC.K1[3]], 1)
        for form in ("seq", "pair"):
            Rg, tg, err = PR.compute_pose(X.tolist(), us.tolist(), PC.K1, form=form)
            assert np.abs(np.array(Rg).reshape(3, 3) - R).max() < 1e-6 and np.abs(np.array(tg) - t).max() < 1e-5 and err < 1e-5


def test_case_list_is_what_the_tests_name():
    assert [c.name for c in PC.all_cases()] == CASE_NAMES
    N = {n: want(n)["N"] for n in CASE_NAMES}
    assert [N[n] for n in CASE_NAMES[:8]] == [9, 10, 11, 21, 63, 64, 65, 257]
    c = cases()["sparse_bad_slots"]
    assert c.n > N["sparse_bad_slots"] and c.bad.any() and (c.kp_point < 0).any() and c.bad[c.kp_point[c.kp_point >= 0]].any()
    assert max(c.n for c in PC.all_cases()) < BATCH_CAP and BATCH_CAP % 64 != 0
    c = cases()["mixed_octaves"]
    assert len(set(int(o) for o in c.octaves[c.kp_point >= 0])) == PC.NLEVELS
    assert cases()["second_camera"].cam[0] != cases()["n64_outliers"].cam[0]


def test_cases_reach_what_they_are_built_for():
    w = want
    a = w("few_9")
    assert a["status"] == PR.FEW | PR.NO_MORE and a["iterations"] == 0 and a["ninliers"] == 0 and not a["pose"]["Tcw"].any()
    a = w("n10_cap_one")                     # N == min: a cap of 1, yet iterate(5) runs 5 (the or); Refine gives 10, not more than 10: mBestTcw
    assert (a["min_inliers"], a["cap"], a["status"], a["iterations"], a["ninliers"]) == (10, 1, PR.FOUND | PR.NO_MORE, 5, 10)
    a = w("n11_clean")
    assert (a["min_inliers"], a["cap"]) == PR.ransac(0.99, 10, 300, 4, 0.5, 11) and a["status"] == PR.FOUND | PR.REFINED and a["returned"] == 0
    assert w("n21_clean")["min_inliers"] == 10 and w("n21_clean")["status"] == PR.FOUND | PR.REFINED and w("n21_clean")["ninliers"] == 21
    for n, k in (("n63_outliers", 2), ("n64_outliers", 2), ("n65_outliers", 2), ("n257_outliers", 3), ("late_success", 7), ("second_camera", 2),
                 ("mixed_octaves", 1), ("sparse_bad_slots", 2)):
        a = w(n)
        assert a["status"] == PR.FOUND | PR.REFINED and a["returned"] == k and a["iterations"] == k + 1, n
        assert a["ninliers"] == int(cases()[n].good_rec.sum()) and a["min_inliers"] == max(10, a["N"] // 2), n
    assert [w(n)["min_inliers"] for n in ("n63_outliers", "n64_outliers", "n65_outliers")] == [31, 32, 32]
    # the or of the loop condition: the first iterate(5) of a solver runs the whole cap
    a = w("heavy_best_at_cap")
    counts = [h[2] for h in PC.hypotheses(cases()["heavy_best_at_cap"])]
    assert a["cap"] == 35 and len(counts) == 35 and a["iterations"] == 35 and cases()["heavy_best_at_cap"].params["niterations"] == 5
    assert a["status"] == PR.FOUND | PR.NO_MORE and a["best_inliers"] == a["ninliers"] == a["min_inliers"] == 20 and counts[3] == counts[9] == 20
    runs = PC.refine_runs(cases()["heavy_best_at_cap"])
    assert len(runs) == 1, "Refine is a pure function of the best set: the second qualifying iteration does not improve it"
    H = PC.hypotheses(cases()["heavy_best_at_cap"])[3]
    assert a["pose"].tobytes() == np.asarray(PC.pose_record(*PR.pose_f32(H[0], H[1]), cases()["heavy_best_at_cap"].cam)).tobytes()
    a = w("heavy_nothing")
    assert a["status"] == PR.NO_MORE and a["iterations"] == 35 and a["best_inliers"] == 0 and not a["inlier"].any()
    # a solver already at its cap runs exactly niterations more
    a = w("at_cap_five_more")
    assert a["cap"] == 35 and a["iterations"] == 40 and len(PC.hypotheses(cases()["at_cap_five_more"])) == 5 and a["status"] == PR.FOUND | PR.NO_MORE
    # the resumed solver: iteration 0 qualifies without improving, Refine runs on the CARRIED set of 25 and returns 30
    c = cases()["resume_carried_best"]
    a = w("resume_carried_best")
    runs = PC.refine_runs(c)
    assert a["min_inliers"] <= PC.hypotheses(c)[0][2] < 30 == c.params["best_inliers_in"] and len(runs) == 1 and int(runs[0][2].sum()) == 25
    assert a["status"] == PR.FOUND | PR.REFINED and a["returned"] == 5 and a["iterations"] == 6 and a["ninliers"] == 30 and a["best_inliers"] == 30
    assert a["best_pose"].tobytes() == np.asarray(c.best_pose_in).tobytes() and np.array_equal(a["best_inlier"], c.best_inlier_in)
    # one flag of a hypothesis hangs on CheckInliers' mixed types
    c = cases()["edge_of_threshold"]
    H, rec = PC.hypotheses(c)[0], PC.records(c)
    dbl = PR.check_inliers(H[0], H[1], rec, c.cam, frozenset(["check_double"]))
    assert list(np.flatnonzero(H[3] != dbl)) == [c.edge_record] and w("edge_of_threshold")["status"] == PR.FOUND | PR.REFINED
    assert w("edge_of_threshold")["ninliers"] == 30 and w("edge_of_threshold")["returned"] == 1
    # Refine returns exactly min at a qualifying iteration (strict >: not returned), a later iteration improves and succeeds
    c = cases()["refine_exactly_min"]
    a, runs, H = w("refine_exactly_min"), PC.refine_runs(c), PC.hypotheses(c)
    assert (a["N"], a["min_inliers"], H[0][2], H[1][2]) == (45, 22, 22, 23) and len(runs) == 2
    rc = [int(PR.check_inliers(r[0], r[1], PC.records(c), c.cam).sum()) for r in runs]
    assert rc == [22, 23] and a["status"] == PR.FOUND | PR.REFINED and a["returned"] == 1 and a["ninliers"] == 23
    # a point at z = 0 under a finite hypothesis: invZc = inf through CheckInliers' float stores, never an inlier
    c = cases()["zero_depth"]
    H, rec = PC.hypotheses(c)[1], PC.records(c)
    x, y, z = rec[c.zero_record][0:3]
    assert np.isfinite(H[0]).all() and np.isfinite(H[1]).all() and ((H[0][6] * x + H[0][7] * y) + H[0][8] * z) + H[1][2] == 0.0
    _, e2 = PR.check_inliers(H[0], H[1], rec, c.cam, want_error=True)
    assert not np.isfinite(e2[c.zero_record]) and not H[3][c.zero_record] and H[2] == 30 and np.isfinite(np.delete(e2, c.zero_record)).all()
    assert w("zero_depth")["status"] == PR.FOUND | PR.REFINED and w("zero_depth")["returned"] == 1 and w("zero_depth")["ninliers"] == 30
    # four coplanar points, then four records of one point: garbage or NaN hypotheses that count nothing worth keeping
    H = PC.hypotheses(cases()["degenerate_draws"])
    assert H[0][2] < 20 and all(x != x for x in H[1][0]) and H[1][2] == 0
    assert w("degenerate_draws")["status"] == PR.FOUND | PR.REFINED and w("degenerate_draws")["returned"] == 2


@pytest.mark.parametrize("name", CASE_NAMES)
def test_scan_form_of_the_stop_rule_equals_the_literal_loop(name):
    a, b = want(name), PC.run_reference(cases()[name], scan=True)
    for k in PC.INT_FIELDS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert a["pose"].tobytes() == b["pose"].tobytes() and a["best_pose"].tobytes() == b["best_pose"].tobytes()


@pytest.mark.parametrize("mutant", PR.MUTANTS)
def test_every_mutant_changes_a_compared_output(mutant):
    for n in CASE_NAMES:
        got = PC.run_reference(cases()[n], mut=frozenset([mutant]))
        if PC.differences(cases()[n], want(n), got, recorded()[n])[0]:
            return
    pytest.fail("no case notices the mutant %s" % mutant)


def test_spread_file_is_current_and_every_case_meets_the_condition():
    rec = recorded()
    assert sorted(rec) == sorted(CASE_NAMES)
    for n in CASE_NAMES:
        now = PC.spread(cases()[n])
        assert now == {k: rec[n][k] for k in now}, "%s: tests/golden/pnp_spread.json is stale (run tests/golden/make_pnp_spread.py)" % n
        assert PC.condition(cases()[n], rec[n]) == [], n


def test_null_context_and_bad_parameters_are_argument_errors():
    from pilotguru_amd import _lib
    L = _lib.lib()
    assert L.pgorb_pnp_solver(*([None] * 2 + [0] + [None] * 2 + [0] + [None] * 13)) == _lib.PGORB_E_ARG
    assert L.pgorb_pnp_solver_batch_device(*([None] * 3 + [1, None, 0] + [None] * 2 + [0] + [None] * 15)) == _lib.PGORB_E_ARG
    import pilotguru_amd as pg
    with pytest.raises(ValueError):
        pg.PnPsolver.check_params("t", 0.99, 10, 300, 3, 0.5, 5.991)
    with pytest.raises(ValueError):
        pg.PnPsolver.check_params("t", 0.99, 10, 1025, 4, 0.5, 5.991)
    with pytest.raises(ValueError):
        pg.PnPsolver.check_params("t", 0.99, 10, 300, 4, 0.5, 5.991, draws=np.zeros((300, 3), np.uint32))


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(1000, 1.2, PC.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=4)
    assert np.array_equal(np.asarray(e.GetScaleSigmaSquares(), f32)[:PC.NLEVELS], PC.SIGMA2)
    yield e
    e.close()


def _check_trace(c, got):
    """every hypothesis of the window: R, t as 12 doubles byte for byte (NaN bit patterns apart: NaN equals NaN), the count exactly"""
    H = PC.hypotheses(c)
    tr = got["trace"]
    bad = []
    for k, (R, t, cnt, _) in enumerate(H):
        w_ = np.array(list(R) + list(t), f64)
        g_ = np.concatenate([tr[k]["R"], tr[k]["t"]])
        same = (w_.view(np.uint64) == g_.view(np.uint64)) | (np.isnan(w_) & np.isnan(g_))
        if not same.all() or int(tr[k]["inliers"]) != cnt or int(tr[k]["flags"]) != 1:
            bad.append(k)
    assert not bad, "%s: hypotheses %s differ from the reference" % (c.name, bad)
    assert not tr[len(H):]["flags"].any() and not tr[len(H):]["inliers"].any(), "entries past the window are zeros"
    return len(H)


def _check(c, w, got, what, spread):
    assert not isinstance(got, int), "%s (%s): error %r" % (c.name, what, got)
    nh = _check_trace(c, got)
    bad, d = PC.differences(c, w, got, spread)
    print("%s (%s): status %d, iterations %d, inliers %d of %d, %d hypotheses byte-equal, scaled differences %s against %s" % (
        c.name, what, got["status"], got["iterations"], got["ninliers"], got["N"], nh, d, PC.bounds(spread)))
    assert not bad, "%s (%s): %s differ from the reference" % (c.name, what, bad)
    assert got["ret"] == w["ninliers"]
    # stricter than the bound: Refine's sums run in the reference's sequential order on the device, so its pose is bit-equal too
    assert np.asarray(w["pose"]).tobytes() == np.asarray(got["pose"]).tobytes(), "%s (%s): Refine's pose is not bit-equal" % (c.name, what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_single_call_equals_the_reference(ext, name):
    _check(cases()[name], want(name), PC.run_gpu(cases()[name], ext), "single call", recorded()[name])


@pytest.mark.gpu
def test_gpu_batch_equals_the_reference_and_its_singles_byte_for_byte(ext):
    """Every case in a batch padded to one cap_per_frame (one call per parameter block) -- and the determinism contract: the same
    bytes on a repeat, on a second stream, with the pairs in another order and in a smaller batch."""
    import torch
    seen = 0
    for grp in PC.batch_groups(PC.all_cases()):
        res = PC.run_gpu_batch(grp, ext, BATCH_CAP)
        for c, r in zip(grp, res):
            _check(c, want(c.name), r, "batched", recorded()[c.name])
            assert r["tail_ok"], "%s: the entries past n are not those of no correspondence" % c.name
            assert PC.run_gpu(c, ext)["raw"] == r["raw"], "%s: the single call and the batch differ" % c.name
        raw = [r["raw"] for r in res]
        assert [r["raw"] for r in PC.run_gpu_batch(grp, ext, BATCH_CAP)] == raw, "a repeated call gives other bytes"
        assert [r["raw"] for r in PC.run_gpu_batch(grp, ext, BATCH_CAP, stream=torch.cuda.Stream())] == raw, "a second stream gives other bytes"
        perm = list(np.random.RandomState(len(grp)).permutation(len(grp)))
        got = PC.run_gpu_batch(grp, ext, BATCH_CAP, order=perm)
        assert [got[perm.index(j)]["raw"] for j in range(len(grp))] == raw, "a pair's result depends on its place in the batch"
        if len(grp) > 2:
            assert [r["raw"] for r in PC.run_gpu_batch(grp[1:3], ext, BATCH_CAP)] == raw[1:3], "a pair's result depends on the batch size"
        seen += len(grp)
    assert seen == len(CASE_NAMES)


@pytest.mark.gpu
def test_gpu_python_mirror_equals_the_single_call(ext):
    import pilotguru_amd as pg

    class F:
        pass
    for name in ("n64_outliers", "heavy_best_at_cap", "few_9"):
        c = cases()[name]
        fr = F()
        fr.ext, fr.N, fr.mvKeysUndistorted = ext, c.n, PC.keypoints(c)[:c.n]
        pts = PC.table(c.points)[:len(c.points)]
        tab = pg.MapPointTable(pts, np.zeros((len(pts), 32), np.uint8), c.bad, np.zeros(len(pts) + 1, np.int32), np.zeros(0, np.uint64))
        s = pg.PnPsolver(fr, PC.camera_record(c.cam), c.kp_point, tab, draws=c.draws)
        p = c.params
        s.SetRansacParameters(p["probability"], p["min_inliers"], p["max_iterations"], p["min_set"], p["epsilon"], p["th2"])
        w = want(name)
        assert (s.N, s.mRansacMinInliers, s.mRansacMaxIts) == (w["N"], w["min_inliers"], w["cap"])
        Tcw, no_more, inl, n = s.iterate(p["niterations"])
        g = PC.run_gpu(c, ext)
        assert n == g["ret"] and np.array_equal(inl.astype(np.uint8), g["inlier"]) and no_more == bool(g["status"] & PR.NO_MORE)
        assert (Tcw is None) == (not g["status"] & PR.FOUND) and s.pose.tobytes() == g["pose"].tobytes()
        assert (s.mnIterations, s.mnBestInliers) == (g["iterations"], g["best_inliers"]) and np.array_equal(s.kp_point_out, g["kp_point_out"])


def _chain_frame_keys(c):
    k = PC.keypoints(c)[:c.n].copy()
    k["angle"] = 0.0
    return k


def test_chain_candidates_are_what_the_chain_test_needs():
    import matcher_reference as MR
    cs, asg, srcs, ex = PC.chain_candidates()
    r = [PC.run_reference(c) for c in cs]
    assert [x["status"] for x in r] == [PR.FOUND | PR.REFINED, PR.FOUND | PR.REFINED, PR.NO_MORE]
    assert [x["returned"] for x in r] == [1, 3, -1] and r[2]["iterations"] == 35 and not r[2]["inlier"].any() and not r[2]["pose"]["Tcw"].any()
    assert all(np.array_equal(c.kps_xy, cs[0].kps_xy) for c in cs) and len({c.kp_point.tobytes() for c in cs}) == 3
    fk = _chain_frame_keys(cs[0])
    for j, c in enumerate(cs):
        assert PC.condition(c, dict(err=0.0)) == []
        nm, m = MR.search_by_bow(ex["kf_desc"][j], ex["kf_keys"][j]["angle"], srcs[j] >= 0, ex["kf_fv"][j], ex["fdesc"], fk["angle"], ex["f_fv"], 0.75, True)
        assert np.array_equal(m, asg[j]) and nm == int((asg[j] >= 0).sum()), "SearchByBoW's reference gives the assignment the candidate was built on"


@pytest.mark.gpu
def test_gpu_relocalisation_chain_on_three_candidates_of_one_lost_frame(ext):
    """pgorb_search_by_bow_batch_device -> pgorb_slots_from_assignment_batch_device -> pgorb_pnp_solver_batch_device ->
    pgorb_pose_optimization_batch_device -> pgorb_search_by_projection_keyframe_pose_batch_device on three candidate key frames of ONE
    lost frame (the pair lists repeat it), nothing downloaded in between (Tracking.cc:1359-1450): the solver reads the slots made of
    SearchByBoW's own d_assigned, d_pose_out and d_kp_point_out go to the optimiser as they are, and its pose and slots to the guided
    search, whose sFound and held keypoints are formed on the device.  Every step against its reference (matcher_reference.py,
    pnp_reference.py, pose_reference.py, tracking_reference.py); a later step's reference reads what the device produced, which
    the step before has compared.  The candidate that ends NO_MORE without a pose contributes nothing downstream: no slot,
    PGORB_PO_FEW, no match of the last search."""
    import torch
    import matcher_reference as MR
    import pose_cases as PoC
    import tracking_cases as TC
    import tracking_reference as TR
    from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, MAP_POINT_DTYPE
    cs, asg_want, srcs, ex = PC.chain_candidates()
    L, h = ext._L, ext._h
    npair, n, cap, W = len(cs), cs[0].n, 97, PC.window_cap(cs[0].params)
    nf, FR = npair + 1, npair                                           # rows 0..2: the key frames; row 3: the lost frame
    bounds = (0.0, 640.0, 0.0, 480.0)
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fk = _chain_frame_keys(cs[0])
    kp = np.zeros((nf, cap), KEYPOINT_DTYPE)
    ds = np.zeros((nf, cap, 32), np.uint8)
    fvn, fvs, fvf, nfv = np.zeros((nf, cap), np.uint32), np.zeros((nf, cap + 1), np.int32), np.zeros((nf, cap), np.uint32), np.zeros(nf, np.int32)
    S = np.full((npair, cap), -1, np.int32)
    for j in range(npair):
        m = len(srcs[j])
        kp[j, :m], ds[j, :m], S[j, :m] = ex["kf_keys"][j], ex["kf_desc"][j], srcs[j]
    kp[FR, :n], ds[FR, :n] = fk, ex["fdesc"]
    for f, fv in enumerate(ex["kf_fv"] + [ex["f_fv"]]):
        nfv[f] = len(fv[0]); fvn[f, :len(fv[0])] = fv[0]; fvs[f, :len(fv[1])] = fv[1]; fvf[f, :len(fv[2])] = fv[2]
    nrow = np.array([len(x) for x in srcs] + [n], np.int32)
    tab = np.zeros(n, MAP_POINT_DTYPE)
    tab["pos"], tab["normal"], tab["min_distance"], tab["max_distance"] = cs[0].points, (0, 0, 1), ex["min_d"], ex["max_d"]
    cams = np.zeros(nf, KF_POSE_DTYPE)
    cams[:] = PC.camera_record(cs[0].cam)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dk, dd, dn, dcam = dev(kp.view(np.uint8).reshape(nf, cap, 28)), dev(ds), dev(nrow), dev(cams.view(np.uint8).reshape(nf, -1))
    pkf, pf, dS = dev(np.arange(npair, dtype=np.int32)), dev(np.full(npair, FR, np.int32)), dev(S)
    dT, dPD, dbad = dev(tab.view(np.uint8).reshape(n, 32)), dev(ex["pdesc"]), dev(np.zeros(n, np.uint8))
    dD = dev(np.stack([c.draws for c in cs]).astype(np.uint32).view(np.int32))
    kv = (dS >= 0).to(torch.uint8).contiguous()
    I32 = lambda *sh: torch.full(sh, -9, dtype=torch.int32, device="cuda")
    gs = torch.empty((nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    gi = torch.full((nf, cap), -7, dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_frame_grid_batch_device(h, p(dk), p(dn), nf, cap, *bounds, p(gs), p(gi), s))
    # 1. SearchByBoW(pKF, mCurrentFrame, vvpMapPointMatches[i]) (Tracking.cc:1359)
    asg, nm = I32(npair, cap), I32(npair)
    ext._check(L.pgorb_search_by_bow_batch_device(h, p(dk), p(dd), p(dn), cap, p(dev(fvn)), p(dev(fvs)), p(dev(fvf)), p(dev(nfv)), p(pkf), p(pf),
                                                 npair, p(kv), 0.75, 1, p(asg), p(nm), s))
    # 2. the assignment back to table indices
    kpp = torch.full((npair, cap), -1, dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_slots_from_assignment_batch_device(h, p(asg), p(dS), cap, p(kpp), cap, npair, s))
    # 3. the PnPsolver (:1367-1420)
    pose1 = torch.full((npair, KF_POSE_DTYPE.itemsize), 7, dtype=torch.uint8, device="cuda")
    inl = torch.full((npair, cap), 9, dtype=torch.uint8, device="cuda")
    kpo, info, ninl = I32(npair, cap), I32(npair, 8), I32(npair)
    ext._check(L.pgorb_pnp_solver_batch_device(h, p(dk), p(dn), cap, p(pf), npair, p(dcam), p(kpp), n, p(dT), None,
                                               PC.params_record(cs[0].params).ctypes.data_as(C.c_void_p), None, None, p(dD), None, None,
                                               p(pose1), p(inl), p(kpo), None, p(info), p(ninl), s))
    # 4. PoseOptimization (:1422) with the loop that drops its outliers (:1427-1429)
    pose2 = torch.zeros((npair, KF_POSE_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    outl = torch.full((npair, cap), 9, dtype=torch.uint8, device="cuda")
    kpo2, nmap, info2, ninl2 = I32(npair, cap), I32(npair), I32(npair, 8), I32(npair)
    chi = torch.zeros((npair, cap), dtype=torch.float32, device="cuda")
    ext._check(L.pgorb_pose_optimization_batch_device(h, p(dk), p(dn), cap, p(pf), npair, p(pose1), p(kpo), n, p(dT), None, 1, p(pose2),
                                                      p(outl), p(kpo2), p(nmap), p(chi), p(info2), p(ninl2), s))
    # 5. SearchByProjection(mCurrentFrame, pKF, sFound, 10, 100) (:1434): held keypoints and sFound formed on the device
    has = (kpo2 >= 0).to(torch.uint8).contiguous()
    found_pt = (torch.zeros((npair, n), dtype=torch.int32, device="cuda").scatter_add_(1, kpo2.clamp(min=0).long(), (kpo2 >= 0).to(torch.int32)) > 0)
    flag = (torch.gather(found_pt, 1, dS.clamp(min=0).long()) & (dS >= 0)).to(torch.uint8).contiguous()
    F32 = lambda: torch.full((npair, cap), 77.0, dtype=torch.float32, device="cuda")
    u5, v5, d5, asg5, nm5 = F32(), F32(), F32(), I32(npair, cap), I32(npair)
    ext._check(L.pgorb_search_by_projection_keyframe_pose_batch_device(
        h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pf), p(pkf), npair, *bounds, p(pose2), p(has), p(dS), p(flag), n, p(dT), p(dPD), p(dbad),
        10.0, 100, 1, p(u5), p(v5), p(d5), p(asg5), p(nm5), s))
    torch.cuda.synchronize()                                             # the first download
    H = lambda t: t.cpu().numpy()
    P1 = np.frombuffer(H(pose1).tobytes(), KF_POSE_DTYPE)
    P2 = np.frombuffer(H(pose2).tobytes(), KF_POSE_DTYPE)
    mps = [TR.MapPoint(i, tab["pos"][i], tab["normal"][i], tab["min_distance"][i], tab["max_distance"][i], ex["pdesc"][i]) for i in range(n)]
    matched = []
    for j, c in enumerate(cs):
        m = len(srcs[j])
        n1, a1 = MR.search_by_bow(ex["kf_desc"][j], ex["kf_keys"][j]["angle"], srcs[j] >= 0, ex["kf_fv"][j], ex["fdesc"], fk["angle"], ex["f_fv"], 0.75, True)
        assert int(nm[j]) == n1 and np.array_equal(H(asg[j, :n]), a1), "%s: SearchByBoW" % c.name
        assert np.array_equal(H(kpp[j, :n]), c.kp_point) and (H(kpp[j, n:]) == -1).all(), "%s: the slots" % c.name
        w = PC.run_reference(c)
        i1 = H(info[j])
        got = dict(status=int(i1[0]), N=int(i1[1]), min_inliers=int(i1[2]), cap=int(i1[3]), iterations=int(i1[4]), ninliers=int(i1[5]),
                   best_inliers=int(i1[6]), returned=int(i1[7]), pose=P1[j], inlier=H(inl[j, :n]), kp_point_out=H(kpo[j, :n]),
                   best_inlier=w["best_inlier"], best_pose=w["best_pose"])
        bad, d = PC.differences(c, w, got, dict(R=0.0, t=0.0))
        assert not bad and int(ninl[j]) == w["ninliers"], "%s: the solver differs from the reference: %s" % (c.name, bad)
        assert (H(inl[j, n:]) == 0).all() and (H(kpo[j, n:]) == -1).all()
        pc = PoC.Case("chain_" + c.name, c.kps_xy, c.octaves, dict(Tcw=P1[j]["Tcw"], Ow=P1[j]["Ow"], fx=P1[j]["fx"], fy=P1[j]["fy"], cx=P1[j]["cx"],
                                                                   cy=P1[j]["cy"]), got["kp_point_out"], c.points)
        r4 = PoC.run_reference(pc, discard=True)
        g4 = PoC.result_of(P2[j], H(outl[j, :n]), H(kpo2[j, :n]), nmap[j], H(chi[j, :n]), H(info2[j]), ninl2[j])
        d4 = PoC.differences(pc, r4, g4, PoC.spread(pc))
        assert not d4, "%s: the pose optimisation differs from the reference: %s" % (c.name, d4)
        # the guided search under the device's pose and slots
        slots = g4["kp_point_out"]
        assert np.array_equal(H(has[j, :n]), (slots >= 0).astype(np.uint8))
        found_ref = np.array([t >= 0 and t in set(slots[slots >= 0].tolist()) for t in srcs[j]], np.uint8)
        assert np.array_equal(H(flag[j, :m]), found_ref) and not H(flag[j, m:]).any()
        fr = TR.Frame(1, fk, ex["fdesc"], bounds, P2[j], TC.SF, TC.log_sf(), TC.NLEVELS)
        r5 = TR.search_by_projection_keyframe(fr, ex["kf_keys"][j], [None if t < 0 else mps[t] for t in srcs[j]], found_ref, slots >= 0, 10.0, 100, True)
        g5 = dict(nmatches=int(nm5[j]), assigned=H(asg5[j, :n]), u=H(u5[j, :m]), v=H(v5[j, :m]), dist3d=H(d5[j, :m]))
        d5_ = TC.differences("kf", r5, g5)
        assert not d5_, "%s: the guided search differs from the reference: %s" % (c.name, d5_)
        matched.append(g5["nmatches"])
        if not w["status"] & PR.FOUND:
            assert g4["status"] & 1 and g4["ret"] == 0 and (slots == -1).all() and g5["nmatches"] == 0 and (g5["assigned"] == -1).all(), \
                "a candidate without a pose contributes nothing downstream"
        else:
            assert g4["ret"] >= w["min_inliers"] and g4["status"] == 0
    assert max(matched) > 0, "the guided search finds further matches for a found candidate"


@pytest.mark.gpu
def test_gpu_limits(ext):
    """A window of 1024 runs; one past it is PGORB_E_LIMIT; min_set != 4 is PGORB_E_ARG."""
    from pilotguru_amd import _lib
    c = cases()["n11_clean"]
    big = PC.Case()
    big.__dict__.update(c.__dict__)
    big.params = dict(c.params, max_iterations=1024)
    big.draws = np.concatenate([c.draws, np.random.RandomState(1).randint(0, 2 ** 31, (1024 - len(c.draws), 4)).astype(np.uint32)])
    g = PC.run_gpu(big, ext)
    assert not isinstance(g, int) and g["status"] == want("n11_clean")["status"] and g["pose"].tobytes() == want("n11_clean")["pose"].tobytes()
    big.params = dict(c.params, max_iterations=1025)
    big.draws = np.concatenate([big.draws, big.draws[:1]])
    assert PC.run_gpu(big, ext) == _lib.PGORB_E_LIMIT
    big.params = dict(c.params, max_iterations=5, niterations=1025)
    assert PC.run_gpu(big, ext) == _lib.PGORB_E_LIMIT
    for ms in (3, 5):
        assert PC.run_gpu(c, ext, min_set=ms) == _lib.PGORB_E_ARG
