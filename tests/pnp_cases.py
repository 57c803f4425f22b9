"""The relocalisation candidates tests/test_pnp_solver.py runs pgorb_pnp_solver on, their reference results (tests/pnp_reference.py),
the recorded spread of Refine's arithmetic forms, and the runners of the single and the batched call.

Every case is small: N is chosen for what it exercises (9: FEW; 10: N == min, cap 1; 11: epsilon raised to 10/11; 21: int(10.5) =
10; 63 / 64 / 65: around the wave width, min becomes N/2; 257: above one workgroup).  Outliers lie at least 20 px from the true
projection and inliers carry at most 0.3 px of noise, so no inlier flag of a Refine hangs on the last bits of an error (condition())."""
import ctypes as C
import json
import os

import numpy as np

import pnp_reference as PR
from sim3_reference import level_sigma2

f32, f64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
SPREAD_FILE = os.path.join(HERE, "golden", "pnp_spread.json")
NLEVELS = 8
SIGMA2 = level_sigma2(1.2, NLEVELS)
ULP1 = float(np.spacing(f32(1.0)))
RELOC = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991,
             first_iteration=0, niterations=5, best_inliers_in=0)
PARAM_KEYS = ("probability", "min_inliers", "max_iterations", "min_set", "epsilon", "th2", "first_iteration", "niterations", "best_inliers_in")
K1 = (520.9, 521.0, 325.1, 249.7)
K2 = (458.654, 457.296, 367.215, 248.375)
TRACE_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("inliers", "<i4"), ("flags", "<i4")])
assert TRACE_DTYPE.itemsize == 104
_cache = {}


def rotation(rv):
    rv = np.asarray(rv, f64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


class Case:
    pass


def window_cap(prm):
    return max(int(prm["max_iterations"]), int(prm["niterations"]))


def encode(pos, size):
    """a raw rand() value that RandomInt maps to `pos` of `size`"""
    r = int((pos + 0.5) * 2147483648.0 / size)
    assert PR.random_int(r, size) == pos
    return r


def draws_for(plan, N, W, rng):
    """[W][4] raw draws: random, but iteration k picks the record indices plan[k] where the plan names one"""
    d = rng.randint(0, 2 ** 31, (W, 4)).astype(np.uint32)
    for k, idx in plan.items():
        avail = list(range(N))
        for j, want in enumerate(idx):
            pos = avail.index(want)
            d[k, j] = encode(pos, len(avail))
            avail[pos] = avail[-1]
            avail.pop()
        assert PR.select_literal(d[k], N) == list(idx)
    return d


def scene(name, seed, n_good, n_out=0, noise=0.0, cam=K1, octaves="zero", sparse=0, nbad=0, plan=None, params=None, coplanar=0, twins=0):
    """A lost frame and one candidate's matches: n_good + n_out correspondences in keypoint order (shuffled), `sparse` keypoints
    without a point and `nbad` with a bad one.  plan(good, out, extra) -> {iteration: record indices}."""
    rng = np.random.RandomState(seed)
    c = Case()
    c.name, c.cam = name, tuple(float(f32(v)) for v in cam)
    R, t = rotation(rng.uniform(-0.4, 0.4, 3)), rng.uniform(-0.5, 0.5, 3) + np.array([0, 0, 5.0])
    N = n_good + n_out
    X = rng.uniform(-2.0, 2.0, (N, 3)).astype(f32)
    if coplanar:                                                        # the first `coplanar` good points share a plane of the world
        X[:coplanar, 2] = f32(0.25)
    if twins:                                                           # four records of one and the same point
        X[coplanar:coplanar + twins] = X[coplanar]
    Xc = X.astype(f64) @ R.T + t
    uv = np.stack([cam[0] * Xc[:, 0] / Xc[:, 2] + cam[2], cam[1] * Xc[:, 1] / Xc[:, 2] + cam[3]], 1)
    octv = np.zeros(N, np.int32) if octaves == "zero" else (np.arange(N) % NLEVELS).astype(np.int32)
    good = np.zeros(N, bool)
    good[:n_good] = True
    obs = uv + rng.normal(size=(N, 2)) * noise * np.sqrt(SIGMA2[octv].astype(f64))[:, None]
    for i in range(n_good, N):                                          # an outlier: anywhere in the image but near its projection
        while True:
            o = rng.uniform([0, 0], [640, 480])
            if np.linalg.norm(o - uv[i]) > 20.0 * np.sqrt(float(SIGMA2[octv[i]])):
                break
        obs[i] = o
    order = rng.permutation(N)
    X, obs, octv, good = X[order], obs[order].astype(f32), octv[order], good[order]
    # keypoints: the N records at increasing keypoint indices among n keypoints; the others hold no point or a bad one
    n = N + sparse + nbad
    slot_kp = np.sort(rng.permutation(n)[:N])
    other = np.setdiff1d(np.arange(n), slot_kp)
    c.n = n
    c.kps_xy = rng.uniform([0, 0], [640, 480], (n, 2)).astype(f32)
    c.octaves = rng.randint(0, NLEVELS, n).astype(np.int32)
    c.kps_xy[slot_kp], c.octaves[slot_kp] = obs, octv
    c.points = np.concatenate([X, rng.uniform(-2, 2, (nbad, 3)).astype(f32)]) if nbad else X
    c.bad = np.zeros(len(c.points), np.uint8)
    c.kp_point = np.full(n, -1, np.int32)
    c.kp_point[slot_kp] = np.arange(N)
    if nbad:
        c.bad[N:] = 1
        c.kp_point[other[:nbad]] = N + np.arange(nbad)
    c.good_rec = good
    c.R, c.t = R, t
    c.params = dict(RELOC, **(params or {}))
    gi, oi = list(np.flatnonzero(good)), list(np.flatnonzero(~good))
    first_co = [int(np.flatnonzero(order == k)[0]) for k in range(coplanar)]
    tw = [int(np.flatnonzero(order == k)[0]) for k in range(coplanar, coplanar + twins)]
    c.best_inlier_in, c.best_pose_in = None, None
    pl = plan(gi, oi, dict(coplanar=first_co, twins=tw)) if plan else {}
    if N >= 4:
        rec = records(c)
        n_min = PR.ransac(*ref_params(c)[:5], N)[0]
        for k in list(pl):
            if isinstance(pl[k], str):                                  # "good": a draw of good records whose hypothesis counts every
                for j in range(400):                                    # good record and nothing else; "qualify": at least min, not all
                    idx = _spread4(gi, j)
                    R_, t_, _ = PR.compute_pose([rec[i][0:3] for i in idx], [rec[i][3:5] for i in idx], c.cam)
                    inl = PR.check_inliers(R_, t_, rec, c.cam)
                    if (pl[k] == "good" and np.array_equal(inl, good)) or (pl[k] == "qualify" and n_min <= int(inl.sum()) < n_good and not inl[~good].any()):
                        pl[k] = idx
                        break
                else:
                    raise RuntimeError("%s: no draw makes iteration %d %s" % (name, k, pl[k]))
    c.draws = draws_for(pl, N, window_cap(c.params), rng) if N >= 4 else rng.randint(0, 2 ** 31, (window_cap(c.params), 4)).astype(np.uint32)
    return c


def _spread4(g, k):
    """four good records spread over the list"""
    return [g[(k * 7 + j * (len(g) // 4)) % len(g)] for j in range(4)]


def all_cases():
    if "cases" in _cache:
        return _cache["cases"]
    bad_then_good = lambda nbad_its: (lambda g, o, e: dict([(k, [o[k % len(o)]] + _spread4(g, k)[:3]) for k in range(nbad_its)] +
                                                           [(nbad_its, "good")]))
    cs = [
        scene("few_9", 1, 9),
        scene("n10_cap_one", 2, 10, plan=lambda g, o, e: {0: "good"}),
        scene("n11_clean", 3, 11, plan=lambda g, o, e: {0: "good"}),
        scene("n21_clean", 4, 21, noise=0.1, plan=lambda g, o, e: {0: "good"}),
        scene("n63_outliers", 5, 44, 19, plan=bad_then_good(2)),
        scene("n64_outliers", 6, 45, 19, plan=bad_then_good(2)),
        scene("n65_outliers", 7, 46, 19, noise=0.3, plan=bad_then_good(2)),
        scene("n257_outliers", 8, 180, 77, plan=bad_then_good(3)),
        scene("late_success", 9, 70, 30, plan=bad_then_good(7)),
        scene("heavy_best_at_cap", 10, 20, 20, plan=lambda g, o, e: {3: "good", 9: "good"}),
        scene("heavy_nothing", 11, 12, 28),
        scene("mixed_octaves", 12, 48, 16, noise=0.3, octaves="all", plan=bad_then_good(1)),
        scene("sparse_bad_slots", 13, 40, 12, sparse=50, nbad=9, plan=bad_then_good(2)),
        scene("degenerate_draws", 14, 40, 10, coplanar=4, twins=4,
              plan=lambda g, o, e: {0: e["coplanar"], 1: e["twins"], 2: "good"}),
        scene("second_camera", 15, 45, 19, cam=K2, plan=bad_then_good(2)),
        scene("at_cap_five_more", 16, 20, 20, params=dict(first_iteration=35, niterations=5), plan=lambda g, o, e: {2: "good"}),
    ]
    cs.append(resume_case())
    cs.append(edge_case())
    cs.append(two_pose_case())
    cs.append(zero_depth_case())
    _cache["cases"] = cs
    return cs


def resume_case():
    """A resumed solver: mnIterations = 5 and a carried best set of 25 of the 30 good records that claims 30 inliers, with its pose.
    Iteration 0 of the call is all good (30 inliers: qualifying, NOT improving), so Refine runs on the CARRIED set and succeeds."""
    c = scene("resume_carried_best", 17, 30, 10, noise=0.3, params=dict(first_iteration=5, niterations=5, best_inliers_in=30),
              plan=lambda g, o, e: {0: "qualify"})
    rec = records(c)
    mask_rec = c.good_rec.copy()
    mask_rec[np.flatnonzero(c.good_rec)[:5]] = False
    c.best_inlier_in = np.zeros(c.n, np.uint8)
    c.best_inlier_in[[rec[e][6] for e in np.flatnonzero(mask_rec)]] = 1
    Rf, tf = PR.pose_f32(list(c.R.reshape(9)), list(c.t))
    c.best_pose_in = pose_record(Rf, tf, c.cam)
    return c


def edge_case():
    """CheckInliers' mixed types decide a flag: under the (garbage) hypothesis of iteration 0 one outlier's observation is placed so
    that `error2 < threshold` as the reference computes it (Xc, Yc, invZc, distX, distY, error2 stored to float) and the same
    comparison in double disagree.  The record is drawn by neither planned iteration, so the hypotheses do not depend on it."""
    c = scene("edge_of_threshold", 18, 30, 10, plan=lambda g, o, e: {0: [o[0]] + _spread4(g, 0)[:3], 1: "good"})
    rec = records(c)
    R, t, _, _ = PR.hypothesis(rec, c.cam, c.draws[0])
    used = set(PR.select_closed(c.draws[0], len(rec))) | set(PR.select_closed(c.draws[1], len(rec)))
    E = [e for e in np.flatnonzero(~c.good_rec) if e not in used][0]
    x, y, z = rec[E][0:3]
    fu, fv, uc, vc = c.cam
    iz = 1.0 / (((R[6] * x + R[7] * y) + R[8] * z) + t[2])
    ue, ve = uc + fu * (((R[0] * x + R[1] * y) + R[2] * z) + t[0]) * iz, vc + fv * (((R[3] * x + R[4] * y) + R[5] * z) + t[1]) * iz
    assert np.isfinite([ue, ve]).all()
    u0 = f32(ue + np.sqrt(float(rec[E][5])))
    us = [u0]
    for _ in range(3000):
        us.append(np.nextafter(us[-1], f32(np.inf)))
    us = [np.nextafter(u0, f32(-np.inf))] + us
    for _ in range(3000):
        us.insert(0, np.nextafter(us[0], f32(-np.inf)))
    vs = [f32(ve + 0.01 * q) for q in range(40)]                        # the crossing moves with v: more chances to fall between
    cand = [(x, y, z, float(u), float(v), rec[E][5], 0) for v in vs for u in us]
    a, b = PR.check_inliers(R, t, cand, c.cam), PR.check_inliers(R, t, cand, c.cam, frozenset(["check_double"]))
    hit = np.flatnonzero(a != b)
    assert len(hit), "no observation separates the mixed types from double"
    c.kps_xy[rec[E][6]] = (cand[hit[0]][3], cand[hit[0]][4])
    c.edge_record = int(E)
    return c


def find_draw(rec, cam, members, target):
    """four records of `members` whose hypothesis counts exactly the records of `target`"""
    for j in range(400):
        idx = _spread4(members, j)
        R_, t_, _ = PR.compute_pose([rec[i][0:3] for i in idx], [rec[i][3:5] for i in idx], cam)
        if np.array_equal(PR.check_inliers(R_, t_, rec, cam), target):
            return idx
    raise RuntimeError("no draw counts exactly the target set")


def two_pose_case():
    """A qualifying iteration whose Refine returns exactly min (not returned), then a later success: 45 records, min = 22; 22 of them
    are consistent with a second pose A, the other 23 with the scene's pose B.  Iteration 0 draws from A: 22 >= 22 becomes the best
    set, Refine on it counts 22, which is not more than 22.  Iteration 1 draws from B: 23 > 22 improves, Refine counts 23."""
    c = scene("refine_exactly_min", 19, 23, 22)
    rec = records(c)
    RA, tA = rotation([0.3, -0.2, 0.25]) @ c.R, c.t + np.array([0.4, -0.3, 0.5])
    for e in np.flatnonzero(~c.good_rec):
        xc = RA @ np.array(rec[e][0:3], f64) + tA
        c.kps_xy[rec[e][6]] = (f32(c.cam[0] * xc[0] / xc[2] + c.cam[2]), f32(c.cam[1] * xc[1] / xc[2] + c.cam[3]))
    rec = records(c)
    A, B = list(np.flatnonzero(~c.good_rec)), list(np.flatnonzero(c.good_rec))
    c.draws = draws_for({0: find_draw(rec, c.cam, A, ~c.good_rec), 1: find_draw(rec, c.cam, B, c.good_rec)}, len(rec), window_cap(c.params),
                        np.random.RandomState(19))
    return c


def zero_depth_case():
    """A point at z = 0 under a hypothesis: under the finite pose of iteration 1 (a good draw) one record's camera depth
    ((R20*X + R21*Y) + R22*Z) + t2 is EXACTLY 0.0 in double, so invZc is inf in its float store, ue / ve and error2 are inf or NaN, and
    the record is not an inlier.  The point is built in three scales -- Z cancels t2 to a float's precision, X the rest to about
    1e-14, Y what is left -- and is drawn by neither planned iteration, so the hypotheses do not depend on it."""
    c = scene("zero_depth", 20, 30, 10, plan=lambda g, o, e: {0: [o[0]] + _spread4(g, 0)[:3], 1: "good"})
    rec = records(c)
    R, t, _, _ = PR.hypothesis(rec, c.cam, c.draws[1])
    assert np.isfinite(R).all() and np.isfinite(t).all()
    used = set(PR.select_closed(c.draws[0], len(rec))) | set(PR.select_closed(c.draws[1], len(rec)))
    E = [e for e in np.flatnonzero(~c.good_rec) if e not in used][0]
    depth = lambda x, y, z: ((R[6] * float(x) + R[7] * float(y)) + R[8] * float(z)) + t[2]
    z = f32(-t[2] / R[8])
    x = f32((-t[2] - R[8] * float(z)) / R[6])
    y0 = f32(((-t[2] - R[8] * float(z)) - R[6] * float(x)) / R[7])
    hit = None
    for dx in range(-3, 4):
        xx = x
        for _ in range(abs(dx)):
            xx = np.nextafter(xx, f32(np.inf if dx > 0 else -np.inf))
        yy = f32(((-t[2] - R[8] * float(z)) - R[6] * float(xx)) / R[7])
        ys = [yy]
        for _ in range(200):
            ys.append(np.nextafter(ys[-1], f32(np.inf)))
            ys.insert(0, np.nextafter(ys[0], f32(-np.inf)))
        for y in ys:
            if depth(xx, y, z) == 0.0:
                hit = (xx, y, z)
                break
        if hit:
            break
    assert hit is not None, "no float point has a depth of exactly 0 under the hypothesis"
    c.points = c.points.copy()
    c.points[c.kp_point[rec[E][6]]] = hit
    c.zero_record = int(E)
    return c


def case(name):
    return {c.name: c for c in all_cases()}[name]


def keypoints(c):
    from pilotguru_amd.orb import KEYPOINT_DTYPE
    k = np.zeros(max(c.n, 1), KEYPOINT_DTYPE)
    k["x"][:c.n], k["y"][:c.n], k["octave"][:c.n] = c.kps_xy[:, 0], c.kps_xy[:, 1], c.octaves
    return k


def records(c):
    kps = [dict(x=c.kps_xy[i, 0], y=c.kps_xy[i, 1], octave=c.octaves[i]) for i in range(c.n)]
    return PR.correspondences(kps, c.kp_point, c.points, c.bad, SIGMA2, c.params["th2"])


def pose_record(Rf, tf, cam):
    from pilotguru_amd.orb import kf_pose
    T = np.zeros((3, 4), f32)
    T[:, :3], T[:, 3] = np.asarray(Rf, f32).reshape(3, 3), np.asarray(tf, f32)
    return kf_pose(T, np.asarray(PR.camera_centre(Rf, tf), f32), *cam)


def camera_record(cam):
    from pilotguru_amd.orb import kf_pose
    return kf_pose(np.zeros((3, 4), f32), np.zeros(3, f32), *cam)


def state_of(c, rec):
    st = PR.State(len(rec))
    st.iterations, st.best_inliers = int(c.params["first_iteration"]), int(c.params["best_inliers_in"])
    if c.best_inlier_in is not None and c.best_pose_in is not None:
        st.best_mask = np.array([bool(c.best_inlier_in[r[6]]) for r in rec], bool)
        T = np.asarray(c.best_pose_in["Tcw"], f32).reshape(3, 4)
        st.best_pose = ([float(x) for x in T[:, :3].reshape(9)], [float(x) for x in T[:, 3]])
    else:
        st.best_inliers = 0
    return st


def ref_params(c):
    p = c.params
    return (p["probability"], p["min_inliers"], p["max_iterations"], p["min_set"], p["epsilon"], p["niterations"])


def hypotheses(c):
    """every hypothesis of the call's window, once per case"""
    key = ("hyps", c.name)
    if key not in _cache:
        rec = records(c)
        n_min, cap = PR.ransac(*ref_params(c)[:5], len(rec))
        W = 0 if len(rec) < n_min else PR.window(cap, int(c.params["first_iteration"]), int(c.params["niterations"]))
        _cache[key] = [PR.hypothesis(rec, c.cam, c.draws[k]) for k in range(W)]
    return _cache[key]


def run_reference(c, mut=frozenset(), form="seq", scan=False):
    rec = records(c)
    hyps = hypotheses(c) if not (set(mut) - {"loop_and", "refine_ge", "refine_current", "improve_ge"}) else None
    if scan:
        r = PR.iterate_scan(rec, c.cam, ref_params(c), c.draws, state_of(c, rec), hyps)
    else:
        r = PR.iterate_literal(rec, c.cam, ref_params(c), c.draws, state_of(c, rec), frozenset(mut), form, hyps)
    return finish(c, rec, r)


def finish(c, rec, r):
    """the reference's result in the library's outputs"""
    kp = np.array([x[6] for x in rec], np.int64)
    out = dict(status=r["status"], N=r["N"], min_inliers=r["min_inliers"], cap=r["cap"], iterations=r["iterations"], ninliers=r["ninliers"],
               best_inliers=r["best_inliers"], returned=r["returned"], refined=r["refined"])
    inl = np.zeros(c.n, np.uint8)
    inl[kp[r["mask"]]] = 1
    out["inlier"] = inl
    if "seen" in r:                                                     # the hypotheses evaluated, as the trace holds them
        out["seen"] = [np.array(list(R) + list(t), f64).tobytes() + bytes([cnt & 255, cnt >> 8]) for R, t, cnt in r["seen"]]
    out["kp_point_out"] = np.where(inl == 1, c.kp_point, -1).astype(np.int32)
    out["pose"] = np.asarray(pose_record(r["pose"][0], r["pose"][1], c.cam) if r["pose"] is not None else np.zeros((), _pose_dtype()))
    st = r["state"]
    few = bool(r["status"] & PR.FEW)
    bi = np.zeros(c.n, np.uint8)
    bi[kp[st.best_mask]] = 1
    out["best_inlier"] = (c.best_inlier_in if c.best_inlier_in is not None else np.zeros(c.n, np.uint8)) if few else bi
    if few:
        out["best_pose"] = np.asarray(c.best_pose_in if c.best_pose_in is not None else np.zeros((), _pose_dtype()))
    else:
        out["best_pose"] = np.asarray(pose_record(st.best_pose[0], st.best_pose[1], c.cam) if st.best_pose is not None else np.zeros((), _pose_dtype()))
    return out


def _pose_dtype():
    from pilotguru_amd.orb import KF_POSE_DTYPE
    return KF_POSE_DTYPE


def reference(c):
    key = ("ref", c.name)
    if key not in _cache:
        _cache[key] = run_reference(c)
    return _cache[key]


INT_FIELDS = ("status", "N", "min_inliers", "cap", "iterations", "ninliers", "best_inliers", "returned", "inlier", "kp_point_out", "best_inlier")


def pose_parts(p):
    T = np.asarray(p["Tcw"], f64).reshape(3, 4)
    return T[:, :3].reshape(9), T[:, 3], np.asarray(p["Ow"], f64)


def scaled_differences(a, b):
    """the largest difference of R (scale 1), t and Ow (scale max(1, |t|)) between two pose records"""
    Ra, ta, oa = pose_parts(a)
    Rb, tb, ob = pose_parts(b)
    s = max(1.0, float(np.abs(ta).max()), float(np.abs(oa).max()))
    return dict(R=float(np.abs(Ra - Rb).max()), t=float(max(np.abs(ta - tb).max(), np.abs(oa - ob).max())) / s)


# ---------------------------------------------------------------- the spread of Refine's forms and the case condition
def spread(c):
    """Between the forms of Refine's long sums ("seq", "pair"): the scaled differences of the returned pose and the largest relative
    difference of error2 over every set Refine ran on.  Raises if the forms disagree in an integer output."""
    a, b = run_reference(c, form="seq"), run_reference(c, form="pair")
    for k in INT_FIELDS:
        if not np.array_equal(np.asarray(a[k]), np.asarray(b[k])):
            raise RuntimeError("%s: the forms disagree in %s" % (c.name, k))
    out = dict(R=0.0, t=0.0, err=0.0)
    if a["status"] & PR.REFINED:
        Ra, ta = a["refined"]
        Rb, tb = b["refined"]
        s = max(1.0, max(abs(x) for x in ta))
        out["R"] = max(abs(x - y) for x, y in zip(Ra, Rb))
        out["t"] = max(abs(x - y) for x, y in zip(ta, tb)) / s
    rec = records(c)
    for (Ra, ta, _), (Rb, tb, _) in zip(refine_runs(c, "seq"), refine_runs(c, "pair")):
        _, ea = PR.check_inliers(Ra, ta, rec, c.cam, want_error=True)
        _, eb = PR.check_inliers(Rb, tb, rec, c.cam, want_error=True)
        ok = np.isfinite(ea) & np.isfinite(eb) & (ea > 0)
        if ok.any():
            out["err"] = max(out["err"], float((np.abs(ea.astype(f64) - eb.astype(f64))[ok] / ea.astype(f64)[ok]).max()))
    return out


def refine_runs(c, form="seq"):
    """(R, t, mask) of every Refine the scan form runs on the case"""
    rec = records(c)
    runs = []
    orig = PR.refine

    def logged(rec_, cam, mask, mut=frozenset(), form_="seq"):
        r = orig(rec_, cam, mask, mut, form)
        runs.append((r[0], r[1], np.asarray(mask).copy()))
        return r
    PR.refine = logged
    try:
        PR.iterate_scan(rec, c.cam, ref_params(c), c.draws, state_of(c, rec), hypotheses(c))
    finally:
        PR.refine = orig
    return runs


def recorded_spread():
    with open(SPREAD_FILE) as f:
        return json.load(f)


def bounds(recorded):
    """Per output of a REFINED pose: the larger of 2 float ulps at the output's scale (the results are floats: two doubles 1e-12 apart
    can land on neighbouring floats) and 16 x the spread recorded between the reference's forms."""
    return {k: max(2.0 * ULP1, 16.0 * float(recorded[k])) for k in ("R", "t")}


def window(recorded):
    return max(4.0 * ULP1, 16.0 * float(recorded["err"]))


def condition(c, recorded):
    """For every set Refine runs on: no correspondence's error2 within the window of its threshold.  Returns what fails."""
    w = window(recorded)
    rec = records(c)
    me = np.array([r[5] for r in rec], f64)
    bad = []
    for R, t, _ in refine_runs(c):
        _, e2 = PR.check_inliers(R, t, rec, c.cam, want_error=True)
        e2 = e2.astype(f64)
        near = np.isfinite(e2) & (np.abs(e2 - me) <= w * me)
        if near.any():
            bad.append("%d correspondences inside the window" % int(near.sum()))
    return bad


def _nan_free(b):
    a = np.frombuffer(b[:96], f64).copy()
    a[np.isnan(a)] = 0.0
    return a.tobytes() + b[96:]


def differences(c, want, got, recorded):
    """The compared outputs that differ.  Integers, flags and masks exactly; a pose that is a hypothesis's (or carried, or zeroed) byte
    for byte; Refine's pose within bounds()."""
    bad = [k for k in INT_FIELDS if not np.array_equal(np.asarray(want[k]), np.asarray(got[k]))]
    if "seen" in want and "seen" in got:                                # two reference runs: the hypotheses both evaluated, byte for byte
        m = min(len(want["seen"]), len(got["seen"]))
        if [_nan_free(x) for x in want["seen"][:m]] != [_nan_free(x) for x in got["seen"][:m]]:
            bad.append("hypotheses")
    if np.asarray(want["best_pose"]).tobytes() != np.asarray(got["best_pose"]).tobytes():
        bad.append("best_pose")
    d = dict(R=0.0, t=0.0)
    if want["status"] & PR.REFINED and got["status"] & PR.REFINED:
        d, b = scaled_differences(want["pose"], got["pose"]), bounds(recorded)
        bad += ["%s %.3g > %.3g" % (k, d[k], b[k]) for k in ("R", "t") if not d[k] <= b[k]]
        for k in ("fx", "fy", "cx", "cy", "invfx", "invfy"):
            if np.asarray(want["pose"][k]).tobytes() != np.asarray(got["pose"][k]).tobytes():
                bad.append(k)
    elif np.asarray(want["pose"]).tobytes() != np.asarray(got["pose"]).tobytes():
        bad.append("pose")
    return bad, d


# ---------------------------------------------------------------- GPU runners
def table(points):
    from pilotguru_amd.orb import MAP_POINT_DTYPE
    pts = np.zeros(max(len(points), 1), MAP_POINT_DTYPE)
    pts["pos"][:len(points)] = points
    return pts


def params_record(prm):
    from pilotguru_amd.orb import PNP_PARAMS_DTYPE
    r = np.zeros(1, PNP_PARAMS_DTYPE)
    for k in PARAM_KEYS:
        r[k] = prm[k]
    return r


def result_of(c, ret, pose, inlier, kpo, best_inlier, best_pose, trace, info):
    return dict(ret=int(ret), status=int(info[0]), N=int(info[1]), min_inliers=int(info[2]), cap=int(info[3]), iterations=int(info[4]),
                ninliers=int(info[5]), best_inliers=int(info[6]), returned=int(info[7]), pose=np.array(pose), inlier=np.array(inlier, np.uint8),
                kp_point_out=np.array(kpo, np.int32), best_inlier=np.array(best_inlier, np.uint8), best_pose=np.array(best_pose),
                trace=np.array(trace),
                raw=b"".join(np.ascontiguousarray(x).tobytes() for x in (pose, inlier, kpo, best_inlier, best_pose, trace, np.asarray(info))))


def run_gpu(c, ext, **kw):
    """The single call through the C ABI."""
    from pilotguru_amd.orb import KF_POSE_DTYPE
    L, h = ext._L, ext._h
    n = c.n
    prm_d = dict(c.params, **kw)
    W = window_cap(prm_d)
    prm = params_record(prm_d)
    pose, bpose = np.zeros(1, KF_POSE_DTYPE), np.zeros(1, KF_POSE_DTYPE)
    pose["fx"] = 9
    fl, kpo, bi = np.full(max(n, 1), 9, np.uint8), np.full(max(n, 1), -9, np.int32), np.full(max(n, 1), 9, np.uint8)
    trace = np.zeros(W, TRACE_DTYPE)
    info = np.full(8, -9, np.int32)
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    k, pts, cam = keypoints(c), table(c.points), np.asarray(camera_record(c.cam)).reshape(1)
    kpp, draws = np.ascontiguousarray(c.kp_point), np.ascontiguousarray(c.draws, np.uint32)
    bin_ = None if c.best_inlier_in is None else np.ascontiguousarray(c.best_inlier_in)
    bpin = None if c.best_pose_in is None else np.asarray(c.best_pose_in).reshape(1)
    ret = L.pgorb_pnp_solver(h, p(k), n, p(cam), p(kpp), len(c.points), p(pts), p(c.bad), p(prm), p(draws), p(bin_), p(bpin), p(pose), p(fl),
                             p(kpo), p(bi), p(bpose), p(trace), p(info))
    if ret < 0:
        return ret
    return result_of(c, ret, pose[0], fl[:n], kpo[:n], bi[:n], bpose[0], trace, info)


def batch_groups(cases):
    """by what one batched call shares: everything in the parameter block but first_iteration and best_inliers_in"""
    groups = {}
    for c in cases:
        groups.setdefault(tuple(c.params[k] for k in PARAM_KEYS if k not in ("first_iteration", "best_inliers_in")), []).append(c)
    return list(groups.values())


def run_gpu_batch(cases, ext, cap, order=None, stream=None):
    """One pgorb_pnp_solver_batch_device over `cases` in `order`, every frame padded to `cap`; the tables are concatenated."""
    import torch
    from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE
    L, h = ext._L, ext._h
    order = list(range(len(cases))) if order is None else list(order)
    cs = [cases[j] for j in order]
    npair = len(cs)
    W = window_cap(cs[0].params)
    kp = np.zeros((npair, cap), KEYPOINT_DTYPE)
    kp["octave"] = 99                                                   # past n: never read
    slots = np.full((npair, cap), 1 << 20, np.int32)
    n = np.zeros(npair, np.int32)
    cams = np.zeros(npair, KF_POSE_DTYPE)
    draws = np.zeros((npair, W, 4), np.uint32)
    bi = np.zeros((npair, cap), np.uint8)
    bp = np.zeros(npair, KF_POSE_DTYPE)
    bin_count = np.zeros(npair, np.int32)
    base, tabs, bads = 0, [], []
    for j, c in enumerate(cs):
        kp[j, :c.n] = keypoints(c)[:c.n]
        slots[j, :c.n] = np.where(c.kp_point >= 0, c.kp_point + base, -1)
        n[j], cams[j], draws[j] = c.n, camera_record(c.cam), c.draws
        if c.best_inlier_in is not None and c.best_pose_in is not None:
            bi[j, :c.n], bp[j], bin_count[j] = c.best_inlier_in, c.best_pose_in, c.params["best_inliers_in"]
        tabs.append(table(c.points)[:len(c.points)])
        bads.append(c.bad)
        base += len(c.points)
    tab, bad = np.concatenate(tabs), np.concatenate(bads)
    st = torch.cuda.current_stream() if stream is None else stream
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    prm = params_record(cs[0].params)
    with torch.cuda.stream(st):
        dk, dn, dcam, dsl, dt, db, dd = dev(kp), dev(n), dev(cams), dev(slots), dev(tab), dev(bad), dev(draws)
        dfi = dev(np.array([c.params["first_iteration"] for c in cs], np.int32))
        dbc, dbi, dbp = dev(bin_count), dev(bi), dev(bp)
        full = lambda shape, dt_: torch.full(shape, 77, dtype=dt_, device="cuda")
        o_pose, o_in, o_kpo = full((npair, KF_POSE_DTYPE.itemsize), torch.uint8), full((npair, cap), torch.uint8), full((npair, cap), torch.int32)
        o_tr, o_info, o_ni = full((npair, W * TRACE_DTYPE.itemsize), torch.uint8), full((npair, 8), torch.int32), full((npair,), torch.int32)
        ext._check(L.pgorb_pnp_solver_batch_device(h, p(dk), p(dn), cap, None, npair, p(dcam), p(dsl), len(tab), p(dt), p(db),
                                                   prm.ctypes.data_as(C.c_void_p), p(dfi), p(dbc), p(dd), p(dbi), p(dbp), p(o_pose), p(o_in),
                                                   p(o_kpo), p(o_tr), p(o_info), p(o_ni), C.c_void_p(st.cuda_stream)))
    st.synchronize()
    pose = np.frombuffer(o_pose.cpu().numpy().tobytes(), KF_POSE_DTYPE)
    bpose = np.frombuffer(dbp.cpu().numpy().tobytes(), KF_POSE_DTYPE)
    trace = np.frombuffer(o_tr.cpu().numpy().tobytes(), TRACE_DTYPE).reshape(npair, W)
    fl, kpo, bio, info, ni = (t.cpu().numpy() for t in (o_in, o_kpo, dbi.view(npair, cap), o_info, o_ni))
    res = []
    for j, c in enumerate(cs):
        r = result_of(c, ni[j], pose[j], fl[j, :c.n], np.where(kpo[j, :c.n] >= 0, kpo[j, :c.n] - (slots[j, :c.n] - c.kp_point), -1),
                      bio[j, :c.n], bpose[j], trace[j], info[j])
        r["tail_ok"] = bool((fl[j, c.n:] == 0).all() and (kpo[j, c.n:] == -1).all())
        res.append(r)
    return res


# ---------------------------------------------------------------- three candidates of one lost frame (the relocalisation hand-off)
def chain_candidates(seed=40, n=90):
    """One lost frame of n keypoints and three candidate key frames whose matches name points of one shared table: candidate 0 and 1
    hold mostly right matches (found at different iterations), candidate 2 mostly wrong ones (NO_MORE without a pose).  Per
    candidate: assigned[i] = the key frame's keypoint SearchByBoW gave frame keypoint i (or -1) and source = that key frame's slots,
    so kp_point = source[assigned] as pgorb_slots_from_assignment forms it.  Returns (cases, assigned, sources, extra); extra holds
    what the searches on either side read: the frame's descriptors (random), per key frame its keypoints and descriptors (the
    matched frame keypoint's with three bits flipped, so SearchByBoW recovers `assigned`), both feature vectors (one node holding
    every feature), and per table point its descriptor (that of the frame keypoint that truly sees it) and distance range."""
    rng = np.random.RandomState(seed)
    R, t = rotation(rng.uniform(-0.4, 0.4, 3)), rng.uniform(-0.5, 0.5, 3) + np.array([0, 0, 5.0])
    X = rng.uniform(-2.0, 2.0, (n, 3)).astype(f32)
    Xc = X.astype(f64) @ R.T + t
    uv = np.stack([K1[0] * Xc[:, 0] / Xc[:, 2] + K1[2], K1[1] * Xc[:, 1] / Xc[:, 2] + K1[3]], 1).astype(f32)
    octv = (np.arange(n) % 3).astype(np.int32)
    cs, asg, srcs = [], [], []
    drng = np.random.RandomState(seed + 1)
    fdesc = drng.randint(0, 256, (n, 32)).astype(np.uint8)
    dist = np.linalg.norm(Xc, axis=1)
    extra = dict(fdesc=fdesc, kf_keys=[], kf_desc=[], kf_fv=[], f_fv=(np.array([7], np.uint32), np.array([0, n], np.int32), np.arange(n, dtype=np.uint32)),
                 pdesc=fdesc.copy(), min_d=(0.5 * dist).astype(f32), max_d=(1.3 * dist).astype(f32))
    for j, (nmatch, nwrong, bad_its) in enumerate(((60, 15, 1), (50, 20, 3), (40, 34, 0))):
        kps = np.sort(rng.permutation(n)[:nmatch])
        point = kps.copy()                                              # the right match: keypoint i sees point i
        wrong = rng.permutation(nmatch)[:nwrong]
        for w in wrong:                                                 # a wrong match: a point that projects at least 20 px away
            while True:
                q = rng.randint(n)
                if np.linalg.norm(uv[q].astype(f64) - uv[kps[w]].astype(f64)) > 40.0:
                    break
            point[w] = q
        m = nmatch + 5                                                  # the key frame: its keypoints in its own order, five without a point
        order = rng.permutation(m)
        source = np.full(m, -1, np.int32)
        source[order[:nmatch]] = point
        assigned = np.full(n, -1, np.int32)
        assigned[kps] = order[:nmatch]
        from pilotguru_amd.orb import KEYPOINT_DTYPE
        kk = np.zeros(m, KEYPOINT_DTYPE)
        kk["x"], kk["y"], kk["octave"] = drng.uniform(20, 620, m), drng.uniform(20, 460, m), drng.randint(0, 3, m)
        kd = drng.randint(0, 256, (m, 32)).astype(np.uint8)
        for i in kps:
            kd[assigned[i]] = fdesc[i]
            for b in drng.permutation(256)[:3]:
                kd[assigned[i], b // 8] ^= np.uint8(1 << (b % 8))
            kk["octave"][assigned[i]] = octv[i]
        extra["kf_keys"].append(kk)
        extra["kf_desc"].append(kd)
        extra["kf_fv"].append((np.array([7], np.uint32), np.array([0, m], np.int32), np.arange(m, dtype=np.uint32)))
        c = Case()
        c.name, c.cam, c.n, c.kps_xy, c.octaves, c.points, c.bad = "chain%d" % j, tuple(float(f32(v)) for v in K1), n, uv, octv, X, np.zeros(n, np.uint8)
        c.kp_point = np.where(assigned >= 0, source[np.maximum(assigned, 0)], -1).astype(np.int32)
        c.params, c.best_inlier_in, c.best_pose_in, c.R, c.t = dict(RELOC), None, None, R, t
        rec = records(c)
        good = np.array([r[6] == c.kp_point[r[6]] for r in rec], bool)
        c.good_rec = good
        gi, oi = list(np.flatnonzero(good)), list(np.flatnonzero(~good))
        plan = dict((k, [oi[k % len(oi)]] + _spread4(gi, k)[:3]) for k in range(bad_its))
        if len(gi) >= 20:
            for jj in range(400):
                idx = _spread4(gi, jj)
                R_, t_, _ = PR.compute_pose([rec[i][0:3] for i in idx], [rec[i][3:5] for i in idx], c.cam)
                if np.array_equal(PR.check_inliers(R_, t_, rec, c.cam), good):
                    plan[bad_its] = idx
                    break
        c.draws = draws_for(plan, len(rec), window_cap(c.params), rng)
        cs.append(c)
        asg.append(assigned)
        srcs.append(source)
    return cs, asg, srcs, extra
