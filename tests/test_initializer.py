"""Initializer (pgorb_initializer, pilotguru_amd/csrc/initializer.hip) against tests/init_reference.py.

The CPU tests anchor the reference independently of the readings it encodes (numpy's SVD, noise-free geometry, the literal
selection list, the literal loop, the mutants); the GPU tests then pin the device to the reference byte for byte: every traced
hypothesis (H, F and both scores as bit patterns with NaN equal to NaN, both counts, the set) and every other output (pose, P3D,
flags, matches12_out, the map, info), with the one exception of finfo's parallaxes, which go through an acos and are compared
within init_cases.parallax_tolerance.  Under init_cases.condition no decision depends on that acos and RH stays 0.02 away from
0.40, so the exact 0.40 edge of the model choice is NOT exercised here.
"""
import functools
import json
import re
import types

import numpy as np
import pytest

from tests import init_cases as IC
from tests import init_reference as IR

f32, f64 = np.float32, np.float64
CASE_NAMES = ["few_7", "n8_all", "n9", "n63", "n64", "n65", "n257", "planar_64", "planar_120", "planar_257", "general_ok", "general_200",
              "rotation_only", "tiny_baseline", "identical", "uneven_frames", "gaps", "collinear_set", "twin_set", "same8_set", "good_50",
              "good_51", "good_52", "planar_good_50", "planar_good_51", "ninety_percent", "behind_half", "one_iteration", "singular_h", "no_model"]
BATCH_CAP = 333                                                          # no multiple of 64, above the largest frame

# what each case is built for: the status word exactly, and (where it matters) nGood of the examined hypothesis
H_, F_ = IR.MODEL_H, IR.MODEL_F
EXPECT = {
    "few_7": IR.FEW, "n8_all": F_ | IR.AMBIGUOUS | IR.FEW_GOOD, "n9": F_ | IR.FEW_GOOD, "n63": F_ | IR.FEW_GOOD, "n64": F_ | IR.FEW_GOOD,
    "n65": F_ | IR.OK, "n257": F_ | IR.FEW_GOOD, "planar_64": H_ | IR.OK, "planar_120": H_ | IR.AMBIGUOUS, "planar_257": H_ | IR.AMBIGUOUS,
    "general_ok": F_ | IR.OK, "general_200": F_ | IR.OK, "rotation_only": H_ | IR.AMBIGUOUS | IR.LOW_PARALLAX,
    "tiny_baseline": H_ | IR.AMBIGUOUS | IR.LOW_PARALLAX, "identical": H_ | IR.DEGENERATE_H, "uneven_frames": F_ | IR.FEW_GOOD,
    "gaps": F_ | IR.OK, "collinear_set": F_ | IR.OK, "twin_set": F_ | IR.FEW_GOOD, "same8_set": F_ | IR.FEW_GOOD, "good_50": F_ | IR.OK,
    "good_51": F_ | IR.OK, "good_52": F_ | IR.OK, "planar_good_50": H_ | IR.AMBIGUOUS | IR.FEW_GOOD, "planar_good_51": H_ | IR.AMBIGUOUS,
    "ninety_percent": F_ | IR.OK, "behind_half": F_ | IR.AMBIGUOUS | IR.FEW_GOOD, "one_iteration": F_ | IR.FEW_GOOD,
    "singular_h": F_ | IR.FEW_GOOD, "no_model": IR.NO_MODEL,
}


@functools.lru_cache(None)
def cases():
    return {c.name: c for c in IC.build()}


@functools.lru_cache(None)
def want(name):
    return IC.run(cases()[name])


@functools.lru_cache(None)
def recorded():
    with open(IC.SPREAD_FILE) as f:
        return json.load(f)


# ---------------------------------------------------------------- CPU: the boundary
def test_symbols_and_mirror_exist():
    import os
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    L = _lib.lib()
    for s in ("pgorb_initializer", "pgorb_initializer_batch_device"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert pg.INIT_PARAMS_DTYPE.itemsize == 16 and pg.INIT_HYPOTHESIS_DTYPE.itemsize == 120
    assert (pg.INIT_FEW, pg.INIT_NO_MODEL, pg.INIT_MODEL_H, pg.INIT_MODEL_F, pg.INIT_OK, pg.INIT_DEGENERATE_H, pg.INIT_AMBIGUOUS, pg.INIT_FEW_GOOD,
            pg.INIT_LOW_PARALLAX) == (IR.FEW, IR.NO_MODEL, IR.MODEL_H, IR.MODEL_F, IR.OK, IR.DEGENERATE_H, IR.AMBIGUOUS, IR.FEW_GOOD, IR.LOW_PARALLAX)
    assert (pg.INIT_INFO, pg.INIT_FINFO, pg.INIT_MAX_ITERATIONS) == (IR.INFO, IR.FINFO, IR.MAX_ITERATIONS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pgorb.h")).read()
    for name, v in (("FEW", 1), ("NO_MODEL", 2), ("MODEL_H", 4), ("MODEL_F", 8), ("OK", 16), ("DEGENERATE_H", 32), ("AMBIGUOUS", 64), ("FEW_GOOD", 128),
                    ("LOW_PARALLAX", 256), ("INFO", IR.INFO), ("FINFO", IR.FINFO), ("MAX_ITERATIONS", 1024)):
        assert re.search(r"#define PGORB_INIT_%s\s+%d\b" % (name, v), hdr), name
    hpp = open(os.path.join(root, "pilotguru_amd", "host", "orb_extractor.hpp")).read()
    assert "class Initializer" in hpp and "pgorb_initializer(" in hpp
    assert hasattr(pg.Initializer, "Initialize") and hasattr(pg.Initializer, "initialize_batch_device")


def test_null_context_and_bad_parameters_are_argument_errors():
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    L = _lib.lib()
    assert L.pgorb_initializer(*([None] * 2 + [0, None, 0] + [None] * 18)) == _lib.PGORB_E_ARG
    assert L.pgorb_initializer_batch_device(*([None] * 3 + [1, None, None, 0] + [None] * 19)) == _lib.PGORB_E_ARG
    for bad in (dict(sigma=0.0), dict(sigma=float("nan")), dict(iterations=0), dict(iterations=1025), dict(draws=np.zeros((200, 7), np.uint32)),
                dict(draws=np.full((200, 8), 2 ** 31, np.int64))):
        with pytest.raises(ValueError):
            pg.Initializer.check_params("t", **dict(dict(sigma=1.0, iterations=200), **bad))


# ---------------------------------------------------------------- CPU: the reference against independent anchors
def _rows(M):
    return [[f32(x) for x in r] for r in M]


@pytest.mark.parametrize("shape", [(16, 9), (9, 8), (3, 3), (4, 4)])
def test_jacobi_against_numpy(shape):
    """the float Jacobi on well-separated spectra: singular values and right vectors of numpy's SVD, up to sign"""
    m, n = shape
    rng = np.random.RandomState(m * 31 + n)
    U, _ = np.linalg.qr(rng.normal(size=(m, m)))
    V, _ = np.linalg.qr(rng.normal(size=(n, n)))
    s = np.linspace(5.0, 1.0, min(m, n))
    A = (U[:, :len(s)] * s) @ V[:len(s), :]
    A = A.astype(f32)
    with np.errstate(all="ignore"):
        At = _rows(A.T)                                                     # n rows of length m
        Vt = [[f32(0)] * n for _ in range(n)]
        W = IR.jacobi(At, Vt)
    _, s_np, vt_np = np.linalg.svd(A.astype(f64))
    k = len(s)
    assert np.allclose(np.array(W, f64)[:k], s_np[:k], rtol=0, atol=2e-6)
    got = np.array(Vt, f64)[:k]
    assert np.allclose(np.abs(np.sum(got * vt_np[:k], 1)), 1.0, atol=1e-5)


def test_completion_vector_of_the_8x9_system():
    c = IC.scene("completion", 40, outliers=0, noise=0.0)
    with np.errstate(all="ignore"):
        prep = IR.prepare(c.k1, c.k2, list(c.matches12))
        sel = list(range(8))
        p1 = [prep["pn1"][prep["i1"][k]] for k in sel]
        p2 = [prep["pn2"][prep["i2"][k]] for k in sel]
        rows = [[u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, f32(1)] for (u1, v1), (u2, v2) in zip(p1, p2)]
        A = np.array(rows, f64)
        W = IR.jacobi(rows)
        IR.complete(rows, W, 9)
    M = np.array(rows, f64)
    v = M[8]
    assert abs(np.linalg.norm(v) - 1.0) < 1e-6 and np.abs(M[:8] @ v).max() < 1e-6
    assert np.abs(A @ v).max() < 1e-5                                       # the null vector of a noise-free 8-point system
    r = IR.RNG()
    assert [1 if (r.next() & 256) else 0 for _ in range(9)] == [0, 0, 1, 0, 0, 0, 0, 1, 1]


def _noise_free(kind, n=40):
    c = IC.scene("anchor_" + kind, n, kind, outliers=0, noise=0.0, iters=4)
    with np.errstate(all="ignore"):
        prep = IR.prepare(c.k1, c.k2, list(c.matches12))
    return c, prep


def test_h21_on_a_noise_free_plane_and_f21_on_a_noise_free_scene():
    c, prep = _noise_free("planar")
    with np.errstate(all="ignore"):
        h = IR.hypothesis(prep, [0, 5, 9, 14, 20, 26, 31, 39], f32(1))
    H = np.array(h["H21"], f64).reshape(3, 3)
    m1 = np.array(prep["m1"], f64)
    m2 = np.array(prep["m2"], f64)
    p = np.c_[m1, np.ones(len(m1))] @ H.T
    assert np.abs(p[:, :2] / p[:, 2:] - m2).max() < 2e-2                    # H maps every point of the plane
    assert all(h["inlH"])
    # H is proportional to K (R + t n^T / d) K^-1 with the plane n.X = d that the scene was built on
    K = np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1.0]])
    X = c.X
    nd = np.linalg.lstsq(X, np.ones(len(X)), rcond=None)[0]                 # n/d
    Ht = K @ (c.R + np.outer(c.t, nd)) @ np.linalg.inv(K)
    assert np.abs(H / H[2, 2] - Ht / Ht[2, 2]).max() < 2e-3 * np.abs(Ht / Ht[2, 2]).max()
    c, prep = _noise_free("general")
    with np.errstate(all="ignore"):
        h = IR.hypothesis(prep, [0, 5, 9, 14, 20, 26, 31, 39], f32(1))
    F = np.array(h["F21"], f64).reshape(3, 3)
    m1 = np.c_[np.array(prep["m1"], f64), np.ones(len(prep["m1"]))]
    m2 = np.c_[np.array(prep["m2"], f64), np.ones(len(prep["m2"]))]
    l2 = m1 @ F.T
    dist = np.abs(np.sum(m2 * l2, 1)) / np.hypot(l2[:, 0], l2[:, 1])
    assert dist.max() < 5e-2 and all(h["inlF"])
    s = np.linalg.svd(F, compute_uv=False)
    assert s[2] < 1e-5 * s[0]                                               # rank 2


def test_initialize_returns_the_generating_motion_on_a_noise_free_scene():
    c = IC.scene("anchor_whole", 60, outliers=0, noise=0.0, iters=8)
    out = IC.run(c)
    assert out["info"][IR.I_STATUS] == IR.MODEL_F | IR.OK and out["ret"] == 60
    P = out["pose"][1][:12].reshape(3, 4).astype(f64)
    assert np.abs(P[:, :3] - c.R).max() < 1e-5
    assert np.abs(P[:, 3] - c.t / np.linalg.norm(c.t)).max() < 1e-4         # the translation up to scale, its sign fixed by the decision
    sel = c.matches12 >= 0
    X = out["P3D"][sel].astype(f64)
    assert np.abs(IC.project(X) - c.k1[sel]).max() < 1e-3
    assert np.abs(IC.project(X @ P[:, :3].T + P[:, 3]) - c.k2[c.matches12[sel]]).max() < 1e-3
    assert np.array_equal(out["pose"][0][:12].reshape(3, 4), np.eye(3, 4, dtype=f32))


def test_closed_form_selection_equals_the_literal_list():
    rng = np.random.RandomState(3)
    for N in (8, 9, 10, 17, 64, 257, 16000):
        rows = [rng.randint(0, 2 ** 31, 8) for _ in range(40)] + [[0] * 8, [2 ** 31 - 1] * 8, [0, 2 ** 31 - 1] * 4, [2 ** 31 - 1, 0] * 4]
        for d8 in rows:
            a, b = IR.select_list(d8, N), IR.select_closed(d8, N)
            assert a == b and len(set(a)) == 8 and all(0 <= x < N for x in a)
    assert sorted(IR.select_list([0] * 8, 8)) == list(range(8))


def test_inverse_of_a_singular_matrix_is_zero():
    with np.errstate(all="ignore"):
        assert IR.inv33([f32(x) for x in (1, 2, 3, 2, 4, 6, 0, 1, 5)]) == [f32(0)] * 9
        got = np.array(IR.inv33([f32(x) for x in (2, 0, 1, 0, 4, 0, 1, 0, 3)]), f64).reshape(3, 3)
    assert np.allclose(got, np.linalg.inv(np.array([[2, 0, 1], [0, 4, 0], [1, 0, 3.0]])), atol=1e-7)


# ---------------------------------------------------------------- CPU: the cases
def test_case_list_is_what_the_tests_name():
    assert sorted(cases()) == sorted(CASE_NAMES) == sorted(EXPECT)
    assert max(max(len(c.k1), len(c.k2)) for c in cases().values()) < BATCH_CAP and BATCH_CAP % 64


def test_cases_reach_what_they_are_built_for():
    for n in CASE_NAMES:
        c, w = cases()[n], want(n)
        I, Fi = w["info"], w["finfo"]
        assert int(I[IR.I_STATUS]) == EXPECT[n], (n, int(I[IR.I_STATUS]))
        assert int(I[IR.I_N]) == c.N and (w["ret"] > 0) == bool(EXPECT[n] & IR.OK)
        if I[IR.I_STATUS] & IR.MODEL_H:
            assert 0.42 < Fi[IR.F_RH] < 0.55, n
        elif I[IR.I_STATUS] & IR.MODEL_F:
            assert Fi[IR.F_RH] < 0.38, n
    g = lambda n: [int(x) for x in want(n)["info"][IR.I_NGOOD:IR.I_NGOOD + 8]]
    ch = lambda n: int(want(n)["info"][IR.I_CHOSEN])
    assert [g(n)[ch(n)] for n in ("good_50", "good_51", "good_52", "planar_good_50", "planar_good_51")] == [50, 51, 52, 50, 51]
    w = want("ninety_percent")
    assert g("ninety_percent")[ch("ninety_percent")] == int(0.9 * int(w["info"][IR.I_MODEL_INL])) == 54
    assert not w["triangulated"][np.flatnonzero(cases()["ninety_percent"].matches12 >= 0)[cases()["ninety_percent"].behind]].any()
    assert sum(1 for x in g("behind_half") if x > 0.7 * max(g("behind_half"))) == 2
    assert int(want("general_ok")["info"][IR.I_INL_F]) >= 56 and int(want("general_200")["info"][IR.I_INL_F]) >= 56
    assert len(want("general_200")["trace"]) == 200 and len(want("one_iteration")["trace"]) == 1
    assert sorted(want("n8_all")["trace"][3]["set"]) == list(range(8))
    u = cases()["uneven_frames"]
    assert len({len(u.k1), len(u.k2), u.N}) == 3
    gp = cases()["gaps"].matches12
    assert any((gp[i:i + 29] == -1).all() for i in range(len(gp) - 29))
    cs = cases()["collinear_set"]
    assert want("collinear_set")["trace"][0]["set"] == list(range(8)) and (cs.draws[1] == 0).all() and (cs.draws[2] == 2 ** 31 - 1).all()
    assert want("collinear_set")["trace"][0]["scoreH"] == 0 and want("twin_set")["trace"][0]["scoreH"] == 0   # degenerate sets: no homography
    tw = cases()["twin_set"]
    i1 = np.flatnonzero(tw.matches12 >= 0)
    assert (tw.k1[i1[0]] == tw.k1[i1[1]]).all() and (tw.k2[tw.matches12[i1[0]]] == tw.k2[tw.matches12[i1[1]]]).all()
    # a singular H21i: the closed-form inverse is the zero matrix, every chi-square is NaN, so is the score, and it never wins
    h0 = want("singular_h")["trace"][0]
    assert h0["set"] == list(range(8)) and IR.inv33(h0["H21"]) == [f32(0)] * 9 and any(x != 0 for x in h0["H21"])
    assert np.isnan(h0["scoreH"]) and all(h0["inlH"]) and int(want("singular_h")["info"][IR.I_BEST_H]) != 0
    # every keypoint of frame 1 in one column: sX is infinite, every hypothesis of both models is NaN, no model is found
    nm = want("no_model")
    assert all(np.isnan(h["scoreH"]) and np.isnan(h["scoreF"]) for h in nm["trace"]) and len(nm["trace"]) == 3
    assert not nm["finfo"].any() and int(nm["info"][IR.I_BEST_H]) == -1 and int(nm["info"][IR.I_BEST_F]) == -1
    idn = want("identical")
    assert int(idn["info"][IR.I_INL_H]) == 90 and int(idn["info"][IR.I_CHOSEN]) == -1


@pytest.mark.parametrize("name", CASE_NAMES)
def test_window_form_equals_the_literal_loop(name):
    a, b = want(name), IC.run(cases()[name], form="loop")
    assert IC.differences(a, b, 0.0) == []


# the cases that notice each mutant (every case is tried; these go first)
NOTICES = {"normalize_matched": "uneven_frames", "score_pairs": "n65", "best_ge": "identical", "f_th_5991": "n65", "f_row8_jacobi": "n9",
           "idx50_no_min": "good_50", "best_good_ge": "planar_good_50", "similar_08": "behind_half", "second_09": "planar_257",
           "t_not_normalised": "good_51"}


@pytest.mark.parametrize("mutant", IR.MUTANTS)
def test_every_mutant_changes_a_compared_output(mutant):
    for n in [NOTICES[mutant]] + [x for x in CASE_NAMES if x != NOTICES[mutant] and x != "general_200"]:
        got = IC.run(cases()[n], mut=(mutant,))
        if IC.differences(want(n), got, recorded()[n]):
            return
    pytest.fail("no case notices the mutant %s" % mutant)


def test_spread_file_is_current_and_every_case_meets_the_condition():
    rec = recorded()
    assert sorted(rec) == sorted(CASE_NAMES)
    for n in CASE_NAMES:
        # the three forms come from this machine's libm through numpy: another build may move one of them by a last bit, so the
        # record is current when it is within 2 float ulps at the case's largest parallax
        par = want(n)["finfo"][IR.F_PARALLAX:]
        ulp = float(np.spacing(f32(np.nanmax(np.abs(par))))) if np.isfinite(par).any() else 0.0
        assert abs(IC.spread(cases()[n], want(n)) - rec[n]) <= 2 * ulp, \
            "%s: tests/golden/init_spread.json is stale (run tests/golden/make_init_spread.py)" % n
        assert IC.condition(cases()[n], want(n)) == [], n


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=4)
    yield e
    e.close()


def _frame(ext, xy):
    import pilotguru_amd as pg
    k = np.zeros(len(xy), pg.KEYPOINT_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    return types.SimpleNamespace(ext=ext, N=len(k), mvKeysUndistorted=k)


def _camera_record():
    import pilotguru_amd as pg
    P = np.zeros(1, pg.KF_POSE_DTYPE)
    P["fx"], P["fy"], P["cx"], P["cy"], P["invfx"], P["invfy"] = IC.CAMERA
    return P[0]


def _single(ext, c):
    """the single call through the Python mirror -> the reference's dict"""
    import pilotguru_amd as pg
    p = c.params
    ini = pg.Initializer(_frame(ext, c.k1), p["sigma"], p["iters"], c.draws, camera=_camera_record(), minParallax=p["min_parallax"],
                         minTriangulated=p["min_tri"])
    ok, R21, t21, vP3D, vbTri = ini.Initialize(_frame(ext, c.k2), c.matches12, trace=True)
    got = dict(ret=ini.ntriangulated, trace=ini.trace, pose=ini.pose.view(f32).reshape(2, 21), P3D=vP3D, triangulated=vbTri.astype(np.uint8),
               matches12_out=ini.matches12_out, info=ini.info, finfo=ini.finfo, points=ini.map["points"]["pos"], kf_point1=ini.map["kf_point1"],
               kf_point2=ini.map["kf_point2"], obs_start=ini.map["obs_start"], obs_frame=ini.map["obs_frame"], obs_idx=ini.map["obs_idx"],
               npoints=ini.map["npoints"])
    assert ok == bool(ini.info[0] & IR.OK) and (R21 is None) == (not ok)
    if ok:
        assert np.array_equal(np.c_[R21, t21].ravel(), got["pose"][1][:12])
        assert not ini.map["points"]["normal"].any() and not ini.map["points"]["min_distance"].any() and not ini.map["points"]["max_distance"].any()
    return got


def _check(name, got, what):
    d = IC.differences(want(name), got, recorded()[name])
    print("%s (%s): status %d, %d hypotheses compared, parallaxes %s against %s" % (
        name, what, int(got["info"][0]), len(want(name)["trace"]), [float(x) for x in got["finfo"][3:]], [float(x) for x in want(name)["finfo"][3:]]))
    assert d == [], "%s (%s): %s differ from the reference" % (name, what, d)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_single_call_equals_the_reference(ext, name):
    _check(name, _single(ext, cases()[name]), "single call")


def _batch(ext, names, cap, stream=None, with_map=True):
    """one batch of the named cases, two frames each -> a list of the reference's dicts"""
    import torch
    import pilotguru_amd as pg
    dev = torch.device("cuda:0")
    groups = {}
    for n in names:                                                      # one call per parameter block (max_iterations is per call)
        p = cases()[n].params
        groups.setdefault((p["sigma"], p["iters"], p["min_parallax"], p["min_tri"]), []).append(n)
    res = {}
    for (sigma, iters, mp, mt), ns in groups.items():
        nf = 2 * len(ns)
        kps = np.zeros((nf, cap), pg.KEYPOINT_DTYPE)
        nn = np.zeros(nf, np.int32)
        m12 = np.full((len(ns), cap), -1, np.int32)
        draws = np.zeros((len(ns), iters, 8), np.uint32)
        cam = np.zeros(nf, pg.KF_POSE_DTYPE)
        cam[:] = _camera_record()
        for q, n in enumerate(ns):
            c = cases()[n]
            for fr, xy in ((2 * q, c.k1), (2 * q + 1, c.k2)):
                kps["x"][fr, :len(xy)], kps["y"][fr, :len(xy)] = xy[:, 0], xy[:, 1]
                kps["x"][fr, len(xy):], kps["y"][fr, len(xy):] = np.nan, np.nan        # entries past n are never read
                nn[fr] = len(xy)
            m12[q, :len(c.matches12)] = c.matches12
            m12[q, len(c.matches12):] = 5                                               # entries past n are those of no match
            draws[q] = c.draws
        t = lambda a: torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1) if a.dtype.fields else a).to(dev)
        f1 = torch.arange(0, nf, 2, dtype=torch.int32, device=dev)
        f2 = f1 + 1
        out = pg.Initializer.initialize_batch_device(ext, t(kps), t(nn), cap, f1, f2, len(ns), t(cam), t(m12), t(draws), sigma=sigma, iterations=iters,
                                                     minParallax=mp, minTriangulated=mt, with_map=with_map, trace=True, stream=stream)
        torch.cuda.synchronize()
        o = {k: v.cpu().numpy() for k, v in out.items()}
        for q, n in enumerate(ns):
            c = cases()[n]
            n1, n2 = len(c.k1), len(c.k2)
            g = dict(ret=int(o["info"][q][IR.I_RET]), trace=o["trace"][q].view(pg.INIT_HYPOTHESIS_DTYPE), pose=o["pose_out"][q].view(f32).reshape(2, 21),
                     P3D=o["P3D"][q][:n1], triangulated=o["triangulated"][q][:n1], matches12_out=o["matches12_out"][q][:n1], info=o["info"][q],
                     finfo=o["finfo"][q], raw={k: v[q].tobytes() for k, v in o.items()})
            assert not o["P3D"][q][n1:].any() and not o["triangulated"][q][n1:].any() and (o["matches12_out"][q][n1:] == -1).all()
            if with_map:
                np_ = int(o["npoints"][q])
                pts = o["points"][q].view(pg.MAP_POINT_DTYPE)
                g.update(points=pts["pos"][:np_], kf_point1=o["kf_point1"][q][:n1], kf_point2=o["kf_point2"][q][:n2], obs_start=o["obs_start"][q][:np_ + 1],
                         obs_frame=o["obs_frame"][q][:2 * np_] - 2 * q, obs_idx=o["obs_idx"][q][:2 * np_], npoints=np_)
                assert not o["points"][q][np_ * pg.MAP_POINT_DTYPE.itemsize:].any() and (o["kf_point1"][q][n1:] == -1).all()
                assert (o["kf_point2"][q][n2:] == -1).all() and (o["obs_start"][q][np_:] == 2 * np_).all() and (o["obs_idx"][q][2 * np_:] == -1).all()
            res[n] = g
    return res


@pytest.mark.gpu
def test_gpu_batch_equals_the_reference_and_its_singles_byte_for_byte(ext):
    import torch
    a = _batch(ext, CASE_NAMES, BATCH_CAP)
    for n in CASE_NAMES:
        _check(n, a[n], "batch")
        s = _single(ext, cases()[n])
        assert IC.differences(s, a[n], 0.0, exact_parallax=True) == [], n
    again = _batch(ext, CASE_NAMES, BATCH_CAP)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        other = _batch(ext, CASE_NAMES, BATCH_CAP, stream=st.cuda_stream)
    perm = [CASE_NAMES[i] for i in np.random.RandomState(5).permutation(len(CASE_NAMES))]
    permuted = _batch(ext, perm, BATCH_CAP)
    small = _batch(ext, CASE_NAMES[3:9], BATCH_CAP)
    for n in CASE_NAMES:
        for what, b in (("repeat", again), ("second stream", other), ("permuted", permuted), ("smaller batch", small)):
            if n in b:
                for k, v in a[n]["raw"].items():
                    if k not in ("obs_frame",):                         # (frame indices move with the pair's place in the batch)
                        assert v == b[n]["raw"][k], (n, what, k)
                assert IC.differences(a[n], b[n], 0.0, exact_parallax=True) == [], (n, what)
    nomap = _batch(ext, CASE_NAMES[:6], BATCH_CAP, with_map=False)
    for n in CASE_NAMES[:6]:
        assert nomap[n]["raw"]["P3D"] == a[n]["raw"]["P3D"] and nomap[n]["raw"]["info"] == a[n]["raw"]["info"]


@pytest.mark.gpu
def test_gpu_map_feeds_the_refresh_and_global_bundle_adjustment_as_it_is(ext):
    """Tracking::CreateInitialMapMonocular's chain on one resident batch with nothing downloaded in between: the batched call's
    slice of a pair (points, obs_start, obs_frame, obs_idx with the BATCH's frame indices) and its two poses go to
    pgorb_refresh_map_points_batch_device and to pgorb_global_bundle_adjustment_device unchanged.  The refresh is compared with
    MapPoint::UpdateNormalAndDepth of tests/map_point_reference.py byte for byte; the bundle adjustment must see exactly two
    edges a point, finish every point and both key frames, keep the fixed reference frame and not raise the total chi-square."""
    import ctypes as C
    import torch
    import pilotguru_amd as pg
    from pilotguru_amd.orb import MP_NORMAL_DEPTH
    from tests import map_point_reference as MR
    names = ["n63", "general_ok", "planar_64", "gaps"]                    # pair 0 fails; the others initialise (F, H, F)
    cap = BATCH_CAP
    dev = torch.device("cuda:0")
    nf = 2 * len(names)
    kps = np.zeros((nf, cap), pg.KEYPOINT_DTYPE)
    nn = np.zeros(nf, np.int32)
    m12 = np.full((len(names), cap), -1, np.int32)
    draws = np.zeros((len(names), 24, 8), np.uint32)
    cam = np.zeros(nf, pg.KF_POSE_DTYPE)
    cam[:] = _camera_record()
    for q, n in enumerate(names):
        c = cases()[n]
        for fr, xy in ((2 * q, c.k1), (2 * q + 1, c.k2)):
            kps["x"][fr, :len(xy)], kps["y"][fr, :len(xy)] = xy[:, 0], xy[:, 1]
            nn[fr] = len(xy)
        m12[q, :len(c.matches12)] = c.matches12
        draws[q] = c.draws
    t = lambda a: torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1) if a.dtype.fields else a).to(dev)
    d_kps, d_n = t(kps), t(nn)
    f1 = torch.arange(0, nf, 2, dtype=torch.int32, device=dev)
    out = pg.Initializer.initialize_batch_device(ext, d_kps, d_n, cap, f1, f1 + 1, len(names), t(cam), t(m12), t(draws), iterations=24)
    info = out["info"].cpu().numpy()
    assert [bool(info[q][0] & IR.OK) for q in range(len(names))] == [False, True, True, True]
    p_ = lambda x: C.c_void_p(x.data_ptr())
    sf = np.asarray(ext.GetScaleFactors(), f32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for q in range(1, len(names)):
        np_ = int(info[q][IR.I_RET])
        assert np_ == int(out["npoints"][q]) and np_ >= 50
        # the pair's slice, as views of the call's own tensors; the two poses go to their frames' rows, every other frame is bad
        d_pts, d_os = out["points"][q], out["obs_start"][q][:np_ + 1]
        d_of, d_oi = out["obs_frame"][q][:2 * np_], out["obs_idx"][q][:2 * np_]
        d_pose = torch.zeros((nf, pg.KF_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        d_pose[2 * q:2 * q + 2] = out["pose_out"][q].reshape(2, -1)
        kf_bad = torch.ones(nf, dtype=torch.uint8, device=dev)
        kf_bad[2 * q:2 * q + 2] = 0
        fixed = torch.zeros(nf, dtype=torch.uint8, device=dev)
        fixed[2 * q] = 1
        status = torch.zeros(np_, dtype=torch.int32, device=dev)
        d_desc = torch.zeros((nf, cap, 32), dtype=torch.uint8, device=dev)
        d_pd = torch.zeros((np_, 32), dtype=torch.uint8, device=dev)
        d_ref = torch.zeros(np_, dtype=torch.int32, device=dev)
        ext._check(ext._L.pgorb_refresh_map_points_batch_device(
            ext._h, p_(d_kps), p_(d_desc), p_(d_n), nf, cap, p_(d_pose), p_(kf_bad), np_, p_(d_pts), p_(d_pd), None, p_(d_os), p_(d_of), p_(d_oi),
            2 * np_, p_(d_ref), np_, None, MP_NORMAL_DEPTH, None, p_(status), stream))
        torch.cuda.synchronize()
        rows = np.frombuffer(d_pts.cpu().numpy().tobytes(), pg.MAP_POINT_DTYPE)[:np_]
        poses = np.frombuffer(d_pose.cpu().numpy().tobytes(), pg.KF_POSE_DTYPE)
        of, oi = d_of.cpu().numpy(), d_oi.cpu().numpy()
        assert (of.reshape(-1, 2) == [2 * q, 2 * q + 1]).all() and (status.cpu().numpy() & MP_NORMAL_DEPTH).all()
        kfs = {f: MR.KeyFrame(kps[f][:nn[f]], np.zeros((nn[f], 32), np.uint8), poses[f]["Ow"]) for f in (2 * q, 2 * q + 1)}
        pos0 = out["P3D"][q].cpu().numpy()
        for k in range(np_):
            assert rows["pos"][k].tobytes() == pos0[oi[2 * k]].tobytes()
            mp = MR.MapPoint(rows["pos"][k], np.zeros(32, np.uint8))
            mp.obs = [(kfs[int(of[2 * k + j])], int(oi[2 * k + j])) for j in range(2)]
            mp.ref = mp.obs[0][0]
            assert MR.update_normal_and_depth(mp, sf, 8)
            assert rows["normal"][k].tobytes() == mp.normal.tobytes() and f32(rows["min_distance"][k]) == mp.min_d and \
                f32(rows["max_distance"][k]) == mp.max_d, (names[q], k)
        res = {}
        for its in (0, 20):
            g = pg.Optimizer.GlobalBundleAdjustment_device(ext, d_kps, d_n, cap, d_pose, np_, d_pts, d_os, d_of, d_oi, d_kf_bad=kf_bad,
                                                           d_kf_fixed_id0=fixed, iterations=its)
            torch.cuda.synchronize()
            res[its] = {k: v.cpu().numpy() for k, v in g.items() if v is not None}
        a, b = res[0], res[20]
        print("%s: %d points, chi2 %.4f -> %.4f, info %s" % (names[q], np_, a["chi2"].astype(f64).sum(), b["chi2"].astype(f64).sum(), list(b["info"])))
        assert not (b["info"][0] & (pg.GBA_NONFINITE | pg.GBA_LIMIT | pg.GBA_NOTHING)) and b["info"][1] == 2 * np_ and b["info"][2] == np_
        assert b["point_done"].all() and b["kf_done"][2 * q:2 * q + 2].all() and not np.delete(b["kf_done"], [2 * q, 2 * q + 1]).any()
        assert np.isfinite(b["chi2"]).all() and b["chi2"].astype(f64).sum() <= a["chi2"].astype(f64).sum()
        pb = np.frombuffer(b["pose_out"].tobytes(), pg.KF_POSE_DTYPE)
        assert pb[2 * q]["Tcw"].tobytes() == poses[2 * q]["Tcw"].tobytes()           # the reference frame (mnId 0) is fixed
        assert np.isfinite(pb[2 * q + 1]["Tcw"]).all() and np.isfinite(b["pos_out"]).all()   # (the scale is free: t21 may move)


@pytest.mark.gpu
def test_gpu_errors_and_limits(ext):
    import pilotguru_amd as pg
    from pilotguru_amd._lib import PGORB_E_ARG, PGORB_E_LIMIT
    c = cases()["n9"]
    cam = _camera_record()

    def call(k1=c.k1, k2=c.k2, m=c.matches12, draws=c.draws, iters=6, sigma=1.0, camera=cam):
        return pg.Initializer(_frame(ext, k1), sigma, iters, draws, camera=camera).Initialize(_frame(ext, k2), m)
    assert call()[0] in (True, False)
    bad_k = c.k1.copy()
    bad_k[3, 0] = np.inf
    bad_m = c.matches12.copy()
    bad_m[0] = len(c.k2)
    bad_cam = cam.copy()
    bad_cam["fx"] = np.nan
    for kw in (dict(k1=bad_k), dict(m=bad_m), dict(camera=bad_cam), dict(sigma=0.0), dict(iters=0), dict(draws=np.full((6, 8), 2 ** 31, np.int64))):
        with pytest.raises(ValueError):
            call(**kw)
    # the library's own checks, past the mirror's
    L, h = ext._L, ext._h
    prm = np.zeros(1, pg.INIT_PARAMS_DTYPE)
    prm["sigma"], prm["max_iterations"], prm["min_parallax"], prm["min_triangulated"] = 1.0, 6, 1.0, 50
    k1, k2 = _frame(ext, c.k1).mvKeysUndistorted, _frame(ext, c.k2).mvKeysUndistorted
    n1, n2 = len(k1), len(k2)
    pose, P3D, tri, mo = np.zeros(2, pg.KF_POSE_DTYPE), np.zeros((n1, 3), f32), np.zeros(n1, np.uint8), np.zeros(n1, np.int32)
    info, finfo = np.zeros(pg.INIT_INFO, np.int32), np.zeros(pg.INIT_FINFO, f32)
    p = lambda a: None if a is None else a.ctypes.data

    def raw(k1=k1, n1=n1, m=c.matches12, prm=prm, draws=c.draws, camera=np.array([cam])):
        return L.pgorb_initializer(h, p(k1), n1, p(k2), n2, p(camera), p(m), p(prm), p(draws), p(pose), p(P3D), p(tri), p(mo), None, None, None, None,
                                   None, None, None, None, p(info), p(finfo))
    assert raw() >= 0
    big_draw = c.draws.copy()
    big_draw[2, 3] = 2 ** 31
    neg = prm.copy()
    neg["sigma"] = -1.0
    none = prm.copy()
    none["max_iterations"] = 0
    for kw in (dict(n1=-1), dict(m=None), dict(m=bad_m), dict(draws=big_draw), dict(prm=neg), dict(prm=none), dict(k1=_frame(ext, bad_k).mvKeysUndistorted)):
        assert raw(**kw) == PGORB_E_ARG, kw
    many = prm.copy()
    many["max_iterations"] = pg.INIT_MAX_ITERATIONS + 1
    assert raw(prm=many, draws=np.zeros((pg.INIT_MAX_ITERATIONS + 1, 8), np.uint32)) == PGORB_E_LIMIT
    kbig = np.zeros(16001, pg.KEYPOINT_DTYPE)
    assert L.pgorb_initializer(h, p(kbig), 16001, p(k2), n2, p(np.array([cam])), p(np.full(16001, -1, np.int32)), p(prm), p(c.draws), p(pose),
                               p(np.zeros((16001, 3), f32)), p(np.zeros(16001, np.uint8)), p(np.zeros(16001, np.int32)), None, None, None, None, None,
                               None, None, None, p(info), p(finfo)) == PGORB_E_LIMIT
